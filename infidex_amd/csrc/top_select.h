// The arithmetic of top_groups' ranking (top_groups.hip.inc): how the slot of a group — field_stats' counters, extreme ranks and limb sums — becomes a
// fixed-width order-preserving COMPOSITE, and how a page of groups is selected by that composite over a table of any cardinality.  Not in the reference: the
// ranking is this project's ("top_groups").
//
// Plain C++ behind TS_FN, no HIP types: compiled into k_top_keys / k_top_hist / k_top_pick / k_top_gather / k_top_page and, unchanged, into a host model that
// builds the keys, walks the whole select serially and compares the page with a plain sort under an exact comparator (tests/models/top_select_model.cpp,
// tests/test_top_select_model.py).  The digit picking is listing_select.h's (ls_pick), the sums and means exact_sum.h's — the functions the engine answers with.
//   class      TS_ROW a group with a member and a figure, TS_NOFIG a group with a member whose figure is none or a NaN, TS_NONE a code without a member
//   figure     F big-endian unsigned words, mirrored (~) when descending: 1 for size, count and the min / max sort rank, 2 for a double sum and for the mean
//              (the order-preserving map of the IEEE bits, -0.0 as 0.0), 4 for an int sum (128-bit two's complement, the sign bit flipped); zero without one
//   tie        rank[code] of the group column's facet tie order: a permutation of the codes, never mirrored — every composite of a table is distinct
//   composite  the bit string [class : 2][figure : 32 F][tie : 32], left-aligned in F + 2 words: compared word by word it is the contract's order, and the
//              codes without a member come behind every row
//   pass p     of P = ceil((34 + 32 F) / w) passes, w = digit_bits: the digit is bits [p w, min((p + 1) w, 34 + 32 F)) of the composite, counted for the
//              composites whose bits in front of it equal the target's prefix
//   target     {prefix: the bits chosen so far, as a composite with zeroes behind them; resid: the position among the composites under the prefix}.  After
//              the last pass prefix IS the composite at the position (resid 0: composites are distinct), so the page is the composites between two of them.
#pragma once
#include "listing_select.h"
#include "exact_sum.h"
#ifndef TS_FN
#define TS_FN __host__ __device__ __forceinline__
#endif
#define TS_BY_SIZE 0
#define TS_BY_COUNT 1
#define TS_BY_MIN 2
#define TS_BY_MAX 3
#define TS_BY_SUM 4
#define TS_BY_MEAN 5
#define TS_BYS 6
#define TS_ROW 0u
#define TS_NOFIG 1u
#define TS_NONE 2u
#define TS_MAX_FIG 4                        // words of the widest figure (an int sum)
#define TS_MAX_WORDS (TS_MAX_FIG + 2)       // of the widest composite: 2 + 128 + 32 = 162 bits
#define TS_NO_RANK 0xFFFFFFFFu              // a slot's smallest rank while it has no value that is not a NaN

struct ts_target { uint32_t prefix[TS_MAX_WORDS]; uint32_t resid, dead; };      // dead: no such position (an empty page)

// words of the figure of `by` over a value column of `kind` (XS_KIND_*; by = TS_BY_SIZE needs none)
TS_FN uint32_t ts_fig_words(uint32_t by, int32_t kind) { return by == TS_BY_SUM ? (kind == XS_KIND_INT ? 4u : 2u) : by == TS_BY_MEAN ? 2u : 1u; }
TS_FN uint32_t ts_key_bits(uint32_t figWords) { return 2u + 32u * figWords + 32u; }
TS_FN uint32_t ts_key_words(uint32_t figWords) { return figWords + 2u; }
TS_FN uint32_t ts_passes(uint32_t figWords, uint32_t digitBits) { return (ts_key_bits(figWords) + digitBits - 1u) / digitBits; }
// where pass p's digit begins and how wide it is (the last one may be narrower)
TS_FN uint32_t ts_digit_start(uint32_t pass, uint32_t digitBits) { return pass * digitBits; }
TS_FN uint32_t ts_digit_width(uint32_t pass, uint32_t digitBits, uint32_t keyBits) { const uint32_t s = pass * digitBits; return keyBits - s < digitBits ? keyBits - s : digitBits; }

// the bits of a double that is not a NaN as an unsigned integer of the same order; -0.0 takes 0.0's place (they compare equal)
TS_FN uint64_t ts_double_key(uint64_t bits) {
    if (bits == 0x8000000000000000ull) bits = 0ull;
    return bits >> 63 ? ~bits : bits | 0x8000000000000000ull;
}
TS_FN bool ts_is_nan(uint64_t bits) { return (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

// The class of a slot under `by`, and its figure in fig[0 .. ts_fig_words) (most significant word first, ascending; zero without one).  c: the slot's four
// counters by class (a table without a value column has its members in c[XS_FINITE]), mx / mn: its largest and smallest rank (mn = TS_NO_RANK: none), S: its
// limb sums; kind, scale, nlimbs: the value column's (exact_sum.h).
TS_FN uint32_t ts_figure(uint32_t by, const uint32_t (&c)[4], uint32_t mx, uint32_t mn, const int64_t* S, int32_t kind, int32_t scale, uint32_t nlimbs, uint32_t (&fig)[TS_MAX_FIG]) {
    for (int i = 0; i < TS_MAX_FIG; i++) fig[i] = 0u;
    const uint32_t size = c[0] + c[1] + c[2] + c[3], count = c[XS_FINITE] + c[XS_PINF] + c[XS_NINF];
    if (!size) return TS_NONE;
    if (by == TS_BY_SIZE) { fig[0] = size; return TS_ROW; }
    if (by == TS_BY_COUNT) { fig[0] = count; return TS_ROW; }
    if (by == TS_BY_MIN || by == TS_BY_MAX) {
        if (!count || mn == TS_NO_RANK) return TS_NOFIG;
        fig[0] = by == TS_BY_MIN ? mn : mx;
        return TS_ROW;
    }
    const XsWide W = xs_recombine(S, nlimbs);
    if (by == TS_BY_SUM && kind == XS_KIND_INT) {
        uint64_t lo; int64_t hi; xs_sum_int128(W, &lo, &hi);
        const uint64_t h = (uint64_t)hi ^ 0x8000000000000000ull;
        fig[0] = (uint32_t)(h >> 32); fig[1] = (uint32_t)h; fig[2] = (uint32_t)(lo >> 32); fig[3] = (uint32_t)lo;
        return TS_ROW;
    }
    if (by == TS_BY_MEAN && !count) return TS_NOFIG;
    const uint64_t b = by == TS_BY_SUM ? xs_sum_bits(W, scale, c[XS_PINF], c[XS_NINF]) : xs_mean_bits(W, scale, count, c[XS_PINF], c[XS_NINF]);
    if (ts_is_nan(b)) return TS_NOFIG;
    const uint64_t k = ts_double_key(b);
    fig[0] = (uint32_t)(k >> 32); fig[1] = (uint32_t)k;
    return TS_ROW;
}
// the composite of (class, figure of figWords words, tie) in key[0 .. figWords + 2): the figure mirrored when descending, the whole shifted up against the class
TS_FN void ts_compose(uint32_t cls, const uint32_t (&fig)[TS_MAX_FIG], uint32_t figWords, bool ascending, uint32_t tie, uint32_t (&key)[TS_MAX_WORDS]) {
    uint32_t L[TS_MAX_FIG + 1];              // the words behind the class: the figure, then the tie
#pragma unroll
    for (uint32_t j = 0; j < TS_MAX_FIG + 1; j++) L[j] = j < figWords ? (cls == TS_ROW && !ascending ? ~fig[j] : fig[j]) : j == figWords ? tie : 0u;
#pragma unroll
    for (uint32_t j = 0; j < TS_MAX_WORDS; j++) {
        const uint32_t hi = j ? L[j - 1] : cls, lo = j <= TS_MAX_FIG ? L[j] : 0u;
        key[j] = j <= figWords + 1u ? (hi << 30) | (lo >> 2) : 0u;
    }
}
// bits [start, start + width) of a composite of nw words (width 1 .. 11)
TS_FN uint32_t ts_digit(const uint32_t* key, uint32_t nw, uint32_t start, uint32_t width) {
    const uint32_t w = start >> 5, b = start & 31u;
    const uint64_t two = ((uint64_t)key[w] << 32) | (w + 1u < nw ? key[w + 1u] : 0u);
    return (uint32_t)(two >> (64u - b - width)) & ((1u << width) - 1u);
}
// the first `start` bits of the composite equal the prefix's
TS_FN bool ts_under_prefix(const uint32_t* key, const uint32_t* prefix, uint32_t start) {
    const uint32_t w = start >> 5, b = start & 31u;
    for (uint32_t j = 0; j < w; j++) if (key[j] != prefix[j]) return false;
    return !b || ((key[w] ^ prefix[w]) >> (32u - b)) == 0u;
}
// the prefix with one digit more: bits [start, start + width) set to digit (they were zero)
TS_FN void ts_extend(uint32_t* prefix, uint32_t nw, uint32_t start, uint32_t width, uint32_t digit) {
    const uint32_t w = start >> 5, b = start & 31u;
    const uint64_t v = (uint64_t)digit << (64u - b - width);
    prefix[w] |= (uint32_t)(v >> 32);
    if (w + 1u < nw) prefix[w + 1u] |= (uint32_t)v;
}
TS_FN int ts_cmp(const uint32_t* a, const uint32_t* b, uint32_t nw) {
    for (uint32_t j = 0; j < nw; j++) if (a[j] != b[j]) return a[j] < b[j] ? -1 : 1;
    return 0;
}
// The page of a request over a table of totalGroups rows: its row count, and the two targets before pass 0 — positions offset and offset + count - 1 under
// the empty prefix, dead for an empty page
TS_FN uint32_t ts_start(uint32_t totalGroups, uint32_t offset, uint32_t limit, ts_target* lo, ts_target* hi) {
    const uint32_t count = offset < totalGroups ? (totalGroups - offset < limit ? totalGroups - offset : limit) : 0u;
    for (int j = 0; j < TS_MAX_WORDS; j++) lo->prefix[j] = hi->prefix[j] = 0u;
    lo->dead = hi->dead = count ? 0u : 1u;
    lo->resid = offset; hi->resid = count ? offset + count - 1u : 0u;
    return count;
}
// One digit more for target t from its histogram of this pass (1 << width bins); a histogram that does not hold the position kills the target
TS_FN void ts_step(ts_target* t, const uint32_t* hist, uint32_t nw, uint32_t start, uint32_t width) {
    if (t->dead) return;
    uint32_t dg = 0, rest = 0;
    if (!ls_pick(hist, 1u << width, t->resid, &dg, &rest)) { t->dead = 1u; return; }
    ts_extend(t->prefix, nw, start, width, dg); t->resid = rest;
}
// composite `key` lies on the page the two resolved targets bound
TS_FN bool ts_on_page(const uint32_t* key, uint32_t nw, const ts_target& lo, const ts_target& hi) {
    return !lo.dead && !hi.dead && ts_cmp(key, lo.prefix, nw) >= 0 && ts_cmp(key, hi.prefix, nw) <= 0;
}
