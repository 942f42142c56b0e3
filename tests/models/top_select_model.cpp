// Host model of top_groups' ranking: infidex_amd/csrc/top_select.h on listing_select.h and exact_sum.h, UNCHANGED, driven serially the way k_top_keys,
// k_top_hist, k_top_pick, k_top_gather and k_top_page drive them — composites, then histogram -> pick -> histogram -> ... for the two targets of a page, the
// gather between the two composites found, the sort — over generated tables of slots, and compared row for row with std::sort under an EXACT comparator that
// never looks at a composite: the class, then the figure as a typed value (an unsigned count or rank, a 128-bit integer, a double), then the tie.
// tests/test_top_select_model.py compiles and runs it.
//   top_select_model      runs every case, prints "OK <pages> <rows compared> <pages inside a tie run> <groups without a figure> <groups without a member>
//                         <empty pages>" or the first mismatch (exit 1)
#define LS_FN static inline
#define XS_FN static inline
#define TS_FN static inline
#include "top_select.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef uint64_t u64;
typedef __int128 i128;
static u64 g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }
static u64 g_pages = 0, g_rows = 0, g_tieRuns = 0, g_noFig = 0, g_noMember = 0, g_emptyPages = 0;

struct Slot { uint32_t c[4] = {0, 0, 0, 0}, mx = 0, mn = TS_NO_RANK; int64_t S[XS_MAX_LIMBS] = {0, 0, 0, 0}; };
struct Table { std::vector<Slot> slot; std::vector<uint32_t> tie; int32_t kind = XS_KIND_INT, scale = 0; uint32_t nlimbs = 1; const char* name = ""; };
// what the exact comparator sees of a group
struct Ref { uint32_t cls, code, tie; uint32_t u; i128 i; double d; };

static double as_double(u64 b) { double d; std::memcpy(&d, &b, 8); return d; }
static u64 as_bits(double d) { u64 b; std::memcpy(&b, &d, 8); return b; }

// the figure of slot s as a typed value, from the slot's own fields: no composite, no ts_figure
static Ref reference(const Table& T, uint32_t g, uint32_t by) {
    const Slot& s = T.slot[g];
    Ref R{}; R.code = g; R.tie = T.tie[g]; R.cls = TS_ROW;
    const uint32_t size = s.c[0] + s.c[1] + s.c[2] + s.c[3], count = s.c[XS_FINITE] + s.c[XS_PINF] + s.c[XS_NINF];
    if (!size) { R.cls = TS_NONE; return R; }
    switch (by) {
    case TS_BY_SIZE: R.u = size; break;
    case TS_BY_COUNT: R.u = count; break;
    case TS_BY_MIN: case TS_BY_MAX: if (!count) R.cls = TS_NOFIG; else R.u = by == TS_BY_MIN ? s.mn : s.mx; break;
    case TS_BY_SUM:
        if (T.kind == XS_KIND_INT) { unsigned __int128 v = 0; for (uint32_t k = 0; k < T.nlimbs; k++) v += (unsigned __int128)(i128)s.S[k] << (32 * k); R.i = (i128)v; }
        else { R.d = as_double(xs_sum_bits(xs_recombine(s.S, T.nlimbs), T.scale, s.c[XS_PINF], s.c[XS_NINF])); if (std::isnan(R.d)) R.cls = TS_NOFIG; }
        break;
    default:
        if (!count) R.cls = TS_NOFIG;
        else { R.d = as_double(xs_mean_bits(xs_recombine(s.S, T.nlimbs), T.scale, count, s.c[XS_PINF], s.c[XS_NINF])); if (std::isnan(R.d)) R.cls = TS_NOFIG; }
    }
    return R;
}
// a before b in the contract's order
static bool before(const Ref& a, const Ref& b, uint32_t by, bool intSum, bool asc) {
    if (a.cls != b.cls) return a.cls < b.cls;
    if (a.cls == TS_ROW) {
        int c;
        if (by == TS_BY_SUM && intSum) c = a.i < b.i ? -1 : a.i > b.i ? 1 : 0;
        else if (by == TS_BY_SUM || by == TS_BY_MEAN) c = a.d < b.d ? -1 : a.d > b.d ? 1 : 0;      // (-0.0 == 0.0)
        else c = a.u < b.u ? -1 : a.u > b.u ? 1 : 0;
        if (c) return asc ? c < 0 : c > 0;
    }
    return a.tie < b.tie;
}

static bool run_page(const Table& T, uint32_t by, bool asc, uint32_t db, uint32_t offset, uint32_t limit, const std::vector<Ref>& want, uint32_t totalGroups,
                     const std::vector<uint32_t>& keys, uint32_t F) {
    const uint32_t gv = (uint32_t)T.slot.size(), nw = ts_key_words(F), bits = ts_key_bits(F), passes = ts_passes(F, db);
    ts_target t[2];
    const uint32_t count = ts_start(totalGroups, offset, limit, &t[0], &t[1]);
    for (uint32_t p = 0; p < passes; p++) {                                  // k_top_hist, k_top_pick
        const uint32_t start = ts_digit_start(p, db), width = ts_digit_width(p, db, bits);
        if (start + width > bits || !width || width > db) { printf("FAIL digit geometry\n"); return false; }
        std::vector<uint32_t> hist(2u << width, 0u);
        for (uint32_t g = 0; g < gv; g++) {
            const uint32_t* k = keys.data() + (size_t)g * nw;
            const uint32_t dg = ts_digit(k, nw, start, width);
            for (int x = 0; x < 2; x++) if (!t[x].dead && ts_under_prefix(k, t[x].prefix, start)) hist[((size_t)x << width) + dg]++;
        }
        for (int x = 0; x < 2; x++) ts_step(&t[x], hist.data() + ((size_t)x << width), nw, start, width);
    }
    std::vector<uint32_t> page;                                              // k_top_gather
    for (uint32_t g = 0; g < gv; g++) if (ts_on_page(keys.data() + (size_t)g * nw, nw, t[0], t[1])) page.push_back(g);
    std::sort(page.begin(), page.end(), [&](uint32_t a, uint32_t b) { return ts_cmp(keys.data() + (size_t)a * nw, keys.data() + (size_t)b * nw, nw) < 0; });      // k_top_page
    const uint32_t expect = offset < totalGroups ? std::min(limit, totalGroups - offset) : 0u;
    bool ok = count == expect && page.size() == expect && (!expect || (!t[0].dead && !t[1].dead && t[0].resid == 0 && t[1].resid == 0));
    for (uint32_t r = 0; ok && r < expect; r++) ok = page[r] == want[offset + r].code;
    if (!ok) {
        printf("FAIL table %s groups %u by %u asc %d bits %u offset %u limit %u: rows %zu, expected %u\n", T.name, gv, by, (int)asc, db, offset, limit, page.size(), expect);
        return false;
    }
    g_pages++; g_rows += expect; if (!expect) g_emptyPages++;
    if (expect && offset) {
        // (the page begins inside a run of equal figures when only the tie parts it from the row before)
        Ref a = want[offset - 1], b = want[offset]; a.tie = b.tie = 0;
        if (!before(a, b, by, T.kind == XS_KIND_INT, asc) && !before(b, a, by, T.kind == XS_KIND_INT, asc)) g_tieRuns++;
    }
    return true;
}

static bool run_table(const Table& T, bool withField) {
    const uint32_t gv = (uint32_t)T.slot.size();
    for (uint32_t by = 0; by < TS_BYS; by++) {
        if (!withField && by != TS_BY_SIZE) continue;
        for (int dir = 0; dir < 2; dir++) {
            const bool asc = dir == 0;
            const uint32_t F = ts_fig_words(by, T.kind), nw = ts_key_words(F);
            std::vector<uint32_t> keys((size_t)gv * nw); std::vector<Ref> want; uint32_t rows = 0;
            for (uint32_t g = 0; g < gv; g++) {                              // k_top_keys
                uint32_t fig[TS_MAX_FIG], key[TS_MAX_WORDS];
                const Slot& s = T.slot[g];
                const uint32_t cls = ts_figure(by, s.c, s.mx, s.mn, s.S, T.kind, T.scale, T.nlimbs, fig);
                ts_compose(cls, fig, F, asc, T.tie[g], key);
                for (uint32_t j = 0; j < TS_MAX_WORDS; j++) { if (j < nw) keys[(size_t)g * nw + j] = key[j]; else if (key[j]) { printf("FAIL composite wider than its words\n"); return false; } }
                const Ref R = reference(T, g, by);
                if (R.cls != cls) { printf("FAIL class of group %u by %u table %s: %u, expected %u\n", g, by, T.name, cls, R.cls); return false; }
                if (cls != TS_NONE) { rows++; want.push_back(R); if (cls == TS_NOFIG) g_noFig++; } else g_noMember++;
            }
            std::sort(want.begin(), want.end(), [&](const Ref& a, const Ref& b) { return before(a, b, by, T.kind == XS_KIND_INT, asc); });
            std::vector<uint32_t> offs = {0u, 1u, rows / 3, rows / 2, rows ? rows - 1 : 0u, rows, rows + 5u, 0x7FFFFFFFu};
            for (int k = 0; k < 3; k++) offs.push_back(rows ? rnd() % rows : 0u);
            for (uint32_t db : {4u, 11u, 4u + rnd() % 8u})
                for (uint32_t off : offs)
                    for (uint32_t lim : {1u, 7u, 1024u})
                        if (!run_page(T, by, asc, db, off, lim, want, rows, keys, F)) return false;
        }
    }
    return true;
}

static std::vector<uint32_t> permutation(uint32_t n) {
    std::vector<uint32_t> p(n); for (uint32_t i = 0; i < n; i++) p[i] = i;
    for (uint32_t i = n; i > 1; i--) std::swap(p[i - 1], p[rnd() % i]);
    return p;
}
// a table whose groups hold members drawn from pool (raw values of a column of `kind`); empty: every emptyEvery-th group has no member
static Table from_pool(const char* name, uint32_t gv, int32_t kind, const std::vector<u64>& pool, uint32_t maxMembers, uint32_t emptyEvery) {
    Table T; T.name = name; T.kind = kind; T.slot.resize(gv); T.tie = permutation(gv);
    XsScale sc; if (!xs_column_scale(pool.data(), pool.size(), kind, &sc)) { printf("FAIL pool %s is not summable\n", name); exit(1); }
    T.scale = sc.scale; T.nlimbs = sc.nlimbs;
    for (uint32_t g = 0; g < gv; g++) {
        if (emptyEvery && g % emptyEvery == emptyEvery - 1) continue;
        const uint32_t members = 1 + rnd() % maxMembers;
        Slot& s = T.slot[g];
        for (uint32_t m = 0; m < members; m++) {
            const uint32_t code = rnd() % pool.size();
            uint32_t neg, limb[XS_MAX_LIMBS];
            const uint32_t cls = xs_limbs(pool[code], kind, T.scale, &neg, limb);
            s.c[cls]++;
            if (cls != XS_NAN) { const uint32_t r = code * 0x01000193u; s.mn = std::min(s.mn, r); s.mx = std::max(s.mx, r); }      // (any rank will do: the select only compares)
            for (int i = 0; i < XS_MAX_LIMBS; i++) s.S[i] += neg ? -(int64_t)limb[i] : (int64_t)limb[i];
        }
    }
    return T;
}

int main() {
    const u64 INF = 0x7FF0000000000000ull, NINF = 0xFFF0000000000000ull, NAN_ = 0x7FF8000000000001ull;
    std::vector<u64> ints = {0, 1, (u64)-1, 7, (u64)-40, 0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull, 1ull << 62, (u64)-(1ll << 62), 0xFFFFFFFFull, 1ull << 32};
    std::vector<u64> normal = {as_bits(0.0), as_bits(-0.0), as_bits(1.5), as_bits(-1.5), as_bits(1e9), as_bits(-1e9), as_bits(0.25), as_bits(12.25), INF, NINF, NAN_, NAN_ | 5};
    std::vector<u64> tiny = {as_bits(0.0), as_bits(-0.0), 1ull, 0x8000000000000001ull, 3ull, 0x8000000000000003ull, 0x000FFFFFFFFFFFFFull, 0x0010000000000000ull, 0x8010000000000000ull, NAN_};
    std::vector<u64> nans = {NAN_};
    for (uint32_t gv : {1u, 2u, 7u, 100u, 2049u}) {
        for (int rep = 0; rep < (gv > 1000 ? 1 : 3); rep++) {
            if (!run_table(from_pool("ints", gv, XS_KIND_INT, ints, 5, rep == 1 ? 3 : 0), true)) return 1;
            if (!run_table(from_pool("normal", gv, XS_KIND_DOUBLE, normal, 4, rep == 2 ? 4 : 0), true)) return 1;
            if (!run_table(from_pool("tiny", gv, XS_KIND_DOUBLE, tiny, 3, rep == 1 ? 2 : 0), true)) return 1;
            if (!run_table(from_pool("nans", gv, XS_KIND_DOUBLE, nans, 3, rep == 1 ? 5 : 0), true)) return 1;
        }
        // all keys equal: one member of one value in every group — the tie alone orders the rows
        std::vector<u64> one = {as_bits(12.25)};
        if (!run_table(from_pool("equal", gv, XS_KIND_DOUBLE, one, 1, 0), true)) return 1;
        // no value column: the slot is the member counter
        Table Z; Z.name = "sizes"; Z.slot.resize(gv); Z.tie = permutation(gv);
        for (uint32_t g = 0; g < gv; g++) Z.slot[g].c[0] = g % 5 == 4 ? 0u : 1u + rnd() % 3u;
        if (!run_table(Z, false)) return 1;
        // no group has a member
        Table E; E.name = "empty"; E.slot.resize(gv); E.tie = permutation(gv);
        if (!run_table(E, false)) return 1;
        // int sums at the ends of 128 bits and around +-2^64, set as limb sums (four limbs: wider than a column's two, to reach the ends)
        Table X; X.name = "int128"; X.kind = XS_KIND_INT; X.nlimbs = 4; X.slot.resize(gv); X.tie = permutation(gv);
        const int64_t edge[][4] = {{0, 0, 0, -(1ll << 31)}, {0xFFFFFFFFll, 0xFFFFFFFFll, 0xFFFFFFFFll, (1ll << 31) - 1}, {0, 0, 1, 0}, {-1, 0, 1, 0}, {1, 0, 1, 0}, {0, 0, -1, 0},
                                   {1, 0, -1, 0}, {-1, 0, -1, 0}, {0, 0, 0, 0}, {-1, 0, 0, 0}, {1, 0, 0, 0}, {0, 1ll << 32, 0, 0}, {0, -(1ll << 32), 0, 0}, {-(1ll << 62), 1ll << 30, 0, 0}};
        for (uint32_t g = 0; g < gv; g++) {
            Slot& s = X.slot[g]; const int64_t* e = edge[(g + rnd() % 2) % 14];
            for (int i = 0; i < 4; i++) s.S[i] = e[i];
            s.c[0] = 1 + rnd() % 2; s.mn = s.mx = rnd();
        }
        if (!run_table(X, true)) return 1;
    }
    printf("OK %llu %llu %llu %llu %llu %llu\n", (unsigned long long)g_pages, (unsigned long long)g_rows, (unsigned long long)g_tieRuns, (unsigned long long)g_noFig, (unsigned long long)g_noMember, (unsigned long long)g_emptyPages);
    return 0;
}
