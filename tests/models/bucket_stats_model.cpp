// Host model of bucket_stats' member walk: infidex_amd/csrc/bucket_stats.h on range_buckets.h and exact_sum.h, all three UNCHANGED.  Random members go through
// bks_member into slots laid out by bks_slots / bks_stride — the adds are the kernel's (sts_add: counters, the two extreme ranks, 64-bit limb sums) as relaxed
// atomics on plain words — from one thread and from eight.  Every slot is then held to a brute-force scan that never looks at a threshold search, a limb or a
// scale: the slot by counting the thresholds at or below the rank one by one, the class from the value itself, the sum as an __int128 of value / 2^scale
// built from frexp.  tests/test_bucket_stats_model.py compiles and runs it plain and under -fsanitize=address,undefined.
//   buckets      1, 2, 8, 255 and 256, thresholds random with runs of equal neighbours (empty buckets), with thr[0] = nanRanks and thr[B] = nvals forced in turn
//   nanRanks     0 and 1
//   value tables int64 of one and two limbs (with INT64_MIN and INT64_MAX); doubles of one, two, three and four limbs with NaN, +-inf and +-0.0
// Prints "OK <cases> <members walked> <slots held> <empty slots> <slots with both infinities>"; any mismatch prints it and exits 1.
#define RB_FN static inline
#define XS_FN static inline
#define BKS_FN static inline
#include "bucket_stats.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <thread>
#include <vector>

typedef __int128 i128;

struct Table { int32_t kind; std::vector<uint64_t> bits; std::vector<uint32_t> rank; XsScale sc; };
static double as_double(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }
static uint64_t as_bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
// the table of `vals` with dense ranks in numeric order, a NaN lowest
static Table table_of(int32_t kind, const std::vector<uint64_t>& vals, uint32_t wantLimbs) {
    Table T; T.kind = kind; T.bits = vals; T.rank.assign(vals.size(), 0);
    auto below = [&](uint64_t a, uint64_t b) {
        if (kind == XS_KIND_INT) return (int64_t)a < (int64_t)b;
        const double x = as_double(a), y = as_double(b);
        return std::isnan(x) ? !std::isnan(y) : (!std::isnan(y) && x < y);
    };
    for (size_t i = 0; i < vals.size(); i++) {
        std::vector<uint64_t> under;
        for (size_t j = 0; j < vals.size(); j++) if (below(vals[j], vals[i])) under.push_back(vals[j]);
        std::sort(under.begin(), under.end(), below);
        uint32_t r = 0;
        for (size_t j = 0; j < under.size(); j++) if (!j || below(under[j - 1], under[j])) r++;
        T.rank[i] = r;
    }
    const bool ok = xs_column_scale(T.bits.data(), T.bits.size(), kind, &T.sc);
    if (!ok || T.sc.nlimbs != wantLimbs) { std::printf("TABLE kind=%d limbs=%u want=%u\n", kind, T.sc.nlimbs, wantLimbs); std::exit(1); }
    return T;
}
// value / 2^scale of a finite value, exactly, without exact_sum.h
static i128 brute_int(const Table& T, uint64_t v) {
    if (T.kind == XS_KIND_INT) return (i128)(int64_t)v;
    const double d = as_double(v);
    if (d == 0.0) return 0;
    int e; const double m = std::frexp(std::fabs(d), &e);
    i128 mant = (i128)(uint64_t)std::ldexp(m, 53);
    int sh = e - 53 - T.sc.scale;
    while (sh < 0) { if (mant & 1) { std::printf("SCALE leaves a bit behind\n"); std::exit(1); } mant >>= 1; sh++; }
    if (sh > 74) { std::printf("BRUTE value beyond 127 bits\n"); std::exit(1); }
    mant <<= sh;
    return d < 0 ? -mant : mant;
}

// the kernel's sts_add on plain words: relaxed atomics
static void model_add(uint32_t* slot, const BksMember& M, uint32_t nlimbs) {
    __atomic_fetch_add(slot + M.cls, 1u, __ATOMIC_RELAXED);
    if (M.rank != RB_NO_RANK) {
        uint32_t old = __atomic_load_n(slot + 5, __ATOMIC_RELAXED);
        while (M.rank < old && !__atomic_compare_exchange_n(slot + 5, &old, M.rank, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
        old = __atomic_load_n(slot + 4, __ATOMIC_RELAXED);
        while (M.rank > old && !__atomic_compare_exchange_n(slot + 4, &old, M.rank, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
    for (uint32_t i = 0; i < nlimbs; i++) {
        const int64_t s = M.neg ? -(int64_t)M.limb[i] : (int64_t)M.limb[i];
        if (s) __atomic_fetch_add((uint64_t*)(slot + BKS_HEAD) + i, (uint64_t)s, __ATOMIC_RELAXED);
    }
}

struct Member { uint32_t brank, code; };
static unsigned long long g_cases = 0, g_members = 0, g_slots = 0, g_empty = 0, g_both = 0;

static void run_case(const Table& T, const std::vector<uint32_t>& thr, uint32_t nanRanks, const std::vector<Member>& mem, int threads) {
    const uint32_t ne = (uint32_t)thr.size(), nl = T.sc.nlimbs, W = bks_stride(nl), ns = bks_slots(ne);
    std::vector<uint64_t> store((bks_slot_words(ne, nl) + 1) / 2, 0);      // 8-byte aligned words; exactly the request's slot words (strides are even)
    uint32_t* S = (uint32_t*)store.data();
    for (uint32_t k = 0; k < ns; k++) S[k * W + 5] = RB_NO_RANK;
    // heap copy of exactly nedges thresholds: a read beyond them is the address sanitizer's
    std::vector<uint32_t> H(thr);
    auto walk = [&](int t) {
        for (size_t i = t; i < mem.size(); i += threads) {
            const BksMember M = bks_member(H.data(), ne, nanRanks, mem[i].brank, T.bits[mem[i].code], T.rank[mem[i].code], T.kind, T.sc.scale);
            if (M.slot >= ns) { std::printf("SLOT %u of %u\n", M.slot, ns); std::exit(1); }
            model_add(S + (size_t)M.slot * W, M, nl);
        }
    };
    if (threads == 1) walk(0);
    else { std::vector<std::thread> th; for (int t = 0; t < threads; t++) th.emplace_back(walk, t); for (auto& x : th) x.join(); }
    // brute force, slot by slot
    struct Want { uint32_t c[4] = {0, 0, 0, 0}, mn = RB_NO_RANK, mx = 0; i128 sum = 0; };
    std::vector<Want> want(ns);
    for (const Member& m : mem) {
        uint32_t j = 0; for (uint32_t i = 0; i < ne; i++) if (thr[i] <= m.brank) j++;
        Want& X = want[m.brank < nanRanks ? ne + 1 : j];
        const uint64_t v = T.bits[m.code]; uint32_t cls = XS_FINITE;
        if (T.kind == XS_KIND_DOUBLE) { const double d = as_double(v); cls = std::isnan(d) ? XS_NAN : std::isinf(d) ? (d > 0 ? XS_PINF : XS_NINF) : XS_FINITE; }
        X.c[cls]++;
        if (cls != XS_NAN) { X.mn = std::min(X.mn, T.rank[m.code]); X.mx = std::max(X.mx, T.rank[m.code]); }
        if (cls == XS_FINITE) X.sum += brute_int(T, v);
    }
    for (uint32_t k = 0; k < ns; k++) {
        const uint32_t* c = want[k].c; const uint32_t mn = want[k].mn, mx = want[k].mx; const i128 sum = want[k].sum;
        const uint32_t* G = S + (size_t)k * W;
        int64_t limbSum[XS_MAX_LIMBS] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < nl; i++) std::memcpy(&limbSum[i], G + BKS_HEAD + 2 * i, 8);
        const XsWide Wd = xs_recombine(limbSum, nl);
        i128 got = 0;
        for (int w = 3; w >= 0; w--) got = (got << 32) | Wd.w[w];
        if (Wd.neg) got = -got;
        const bool same = G[0] == c[0] && G[1] == c[1] && G[2] == c[2] && G[3] == c[3] && G[4] == mx && G[5] == mn && got == sum && !Wd.w[4] && !Wd.w[5];
        if (!same) {
            std::printf("MISMATCH kind=%d limbs=%u edges=%u nanRanks=%u threads=%d slot=%u: counters %u %u %u %u want %u %u %u %u, ranks %u %u want %u %u, sum %s\n", T.kind, nl, ne,
                        nanRanks, threads, k, G[0], G[1], G[2], G[3], c[0], c[1], c[2], c[3], G[5], G[4], mn, mx, got == sum ? "equal" : "differs");
            std::exit(1);
        }
        g_slots++; if (!(c[0] + c[1] + c[2] + c[3])) g_empty++; if (c[2] && c[3]) g_both++;
    }
    g_cases++; g_members += mem.size();
}

int main() {
    std::mt19937_64 rng(20241020);
    auto dbl = [&](std::vector<double> v) { std::vector<uint64_t> b; for (double d : v) b.push_back(as_bits(d)); return b; };
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<Table> tables;
    { std::vector<uint64_t> v; for (int i = -20; i < 45; i++) v.push_back((uint64_t)(int64_t)(i * 37)); tables.push_back(table_of(XS_KIND_INT, v, 1)); }
    { std::vector<uint64_t> v = {(uint64_t)INT64_MIN, (uint64_t)INT64_MAX, 0, 1, (uint64_t)-1ll}; for (int i = 0; i < 60; i++) v.push_back(rng() >> (rng() % 40)); tables.push_back(table_of(XS_KIND_INT, v, 2)); }
    { std::vector<double> v = {nan, inf, -inf, 0.0, -0.0}; for (int i = 1; i < 60; i++) v.push_back((i % 2 ? 0.25 : -0.25) * (double)(rng() % 4000 + 1)); tables.push_back(table_of(XS_KIND_DOUBLE, dbl(v), 1)); }
    { std::vector<double> v = {nan, inf, -inf, 0.0, -0.0, std::ldexp(1.0, -20), std::ldexp(1.0, 39)}; for (int i = 1; i < 60; i++) v.push_back(std::ldexp((double)(rng() % 100000 + 1), -20 + (int)(rng() % 40)) * (i % 3 ? 1 : -1)); tables.push_back(table_of(XS_KIND_DOUBLE, dbl(v), 2)); }
    { std::vector<double> v = {nan, inf, -inf, 0.0, -0.0, std::ldexp(1.0, -30), -std::ldexp(1.0, 50)}; for (int i = 1; i < 60; i++) v.push_back(std::ldexp((double)(rng() % 100000 + 1), -30 + (int)(rng() % 60)) * (i % 3 ? 1 : -1)); tables.push_back(table_of(XS_KIND_DOUBLE, dbl(v), 3)); }
    { std::vector<double> v = {nan, inf, -inf, 0.0, -0.0, -std::ldexp(1.0, -50), std::ldexp(1.0, 55)}; for (int i = 1; i < 60; i++) v.push_back(std::ldexp((double)(rng() % 100000 + 1), -50 + (int)(rng() % 85)) * (i % 3 ? 1 : -1)); tables.push_back(table_of(XS_KIND_DOUBLE, dbl(v), 4)); }
    { std::vector<double> v = {1.5, 2.5, -3.0, 0.0}; tables.push_back(table_of(XS_KIND_DOUBLE, dbl(v), 1)); }      // a table without NaN or infinities
    const uint32_t buckets[] = {1, 2, 8, 255, 256};
    for (const Table& T : tables)
        for (uint32_t B : buckets)
            for (uint32_t nanRanks = 0; nanRanks < 2; nanRanks++)
                for (int shape = 0; shape < 4; shape++) {
                    // the bucket column: nb ranks; shape 0 random thresholds, 1 runs of equal ones over few ranks, 2 thr[0] at its floor, 3 thr[B] = nb
                    const uint32_t ne = B + 1, nb = shape == 1 ? 5 + nanRanks : (uint32_t)(rng() % 600) + 2 + nanRanks;
                    std::vector<uint32_t> thr(ne);
                    for (uint32_t& t : thr) t = nanRanks + (uint32_t)(rng() % (nb - nanRanks + 1));
                    std::sort(thr.begin(), thr.end());
                    if (shape == 2) thr[0] = nanRanks;
                    if (shape == 3) thr[B] = nb;
                    std::vector<Member> mem((size_t)(rng() % 3000) + (shape == 1 ? 0 : 200));
                    for (Member& m : mem) { m.brank = (uint32_t)(rng() % nb); m.code = (uint32_t)(rng() % T.bits.size()); }
                    run_case(T, thr, nanRanks, mem, 1);
                    run_case(T, thr, nanRanks, mem, 8);
                }
    // no member at all, and one member
    run_case(tables[0], {0, 3}, 0, {}, 1);
    run_case(tables[3], {1, 1, 4}, 1, {Member{0, 0}}, 8);
    std::printf("OK %llu %llu %llu %llu %llu\n", g_cases, g_members, g_slots, g_empty, g_both);
    return 0;
}
