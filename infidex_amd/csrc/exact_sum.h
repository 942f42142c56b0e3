// The arithmetic of field_stats' exact sums (stats.hip.inc, host/engine.cpp): how a column's values become integers the device can add in any order, and
// how the added integers become the correctly rounded sum and mean.  Not in the reference: the aggregate is this project's ("field_stats").
//
// Plain C++ behind XS_FN, no HIP types: compiled into k_field_stats and the engine and, unchanged, into a host model that is held to fractions.Fraction and
// math.fsum (tests/models/exact_sum_model.cpp, tests/test_exact_sum_model.py).
//   value      the 8 raw bytes of a distinct value: an int64 (kind 1) or the bit pattern of a double (kind 2)
//   scale      per column, the lowest exponent of a SET mantissa bit over its finite values that are not zero (0 for an int column and for a column without
//              such a value): every finite value is an integer multiple of 2^scale
//   bits       1 + (the highest exponent of a set bit) - scale: the width of the largest |v| / 2^scale;  nlimbs L = ceil(bits / 32), at least 1
//   summable   L <= XS_MAX_LIMBS (4: a spread of 128 binary digits); an int column needs at most 2
//   limbs      of one value: its class (finite, NaN, +inf, -inf), its sign and the L unsigned 32-bit digits of |v| / 2^scale — shifts on integers only
//   sums       per accumulator L signed 64-bit sums S_i of +-limb_i.  A limb is below 2^32, so 2^31 - 1 values cannot carry S_i out of 64 bits, and the
//              order of the additions does not matter.  The exact sum is 2^scale * sum_i S_i * 2^(32 i).
//   answer     the S_i recombined to one wide integer (sign and XS_WIDE_WORDS 32-bit digits), rounded ONCE to nearest-even to a double (beyond the double
//              range: +-inf); the mean by long division of the wide integer by the count with a sticky remainder, rounded once; for an int column the
//              128-bit two's complement sum itself.
#pragma once
#include <stdint.h>
#ifndef XS_FN
#define XS_FN __host__ __device__ __forceinline__
#endif
#define XS_MAX_LIMBS 4
#define XS_KIND_INT 1
#define XS_KIND_DOUBLE 2
#define XS_FINITE 0u                         // the classes of a value, also the order of a slot's four counters
#define XS_NAN 1u
#define XS_PINF 2u
#define XS_NINF 3u
#define XS_WIDE_WORDS 6                      // 32 * (XS_MAX_LIMBS - 1) + 64 = 160 bits hold any recombined sum
#define XS_QUOT_SHIFT_WORDS 3                // the mean divides (wide << 96): at least 65 quotient bits in front of the remainder, whatever the count

struct XsScale { int32_t scale; uint32_t bits, nlimbs; };
struct XsWide { uint32_t w[XS_WIDE_WORDS]; uint32_t neg; };      // magnitude, least significant word first; neg only with a magnitude that is not zero

// the class of raw value v of a column of `kind`; for a finite one *neg and *mag, *e0: |v| = mag * 2^e0 (mag = 0 for a zero)
XS_FN uint32_t xs_unpack(uint64_t v, int32_t kind, uint32_t* neg, uint64_t* mag, int32_t* e0) {
    *neg = (uint32_t)(v >> 63);
    if (kind == XS_KIND_INT) { *mag = *neg ? 0ull - v : v; *e0 = 0; return XS_FINITE; }
    const uint32_t e = (uint32_t)(v >> 52) & 0x7FFu; const uint64_t m = v & 0xFFFFFFFFFFFFFull;
    if (e == 0x7FFu) { *mag = 0; *e0 = 0; return m ? XS_NAN : (*neg ? XS_NINF : XS_PINF); }
    *mag = e ? (m | (1ull << 52)) : m;
    *e0 = e ? (int32_t)e - 1075 : -1074;
    return XS_FINITE;
}
XS_FN int32_t xs_low_bit(uint64_t m) { int32_t k = 0; while (!((m >> k) & 1ull)) k++; return k; }             // m != 0
XS_FN int32_t xs_high_bit(uint64_t m) { int32_t k = 63; while (!((m >> k) & 1ull)) k--; return k; }           // m != 0

// the scale and width of a column of n distinct raw values; false: not exactly summable (the nlimbs it would need is still reported)
XS_FN bool xs_column_scale(const uint64_t* vals, uint64_t n, int32_t kind, XsScale* out) {
    bool any = false; int32_t lo = 0, hi = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t neg; uint64_t mag; int32_t e0;
        if (xs_unpack(vals[i], kind, &neg, &mag, &e0) != XS_FINITE || !mag) continue;
        const int32_t l = kind == XS_KIND_INT ? 0 : e0 + xs_low_bit(mag), h = e0 + xs_high_bit(mag);
        if (!any || l < lo) lo = l;
        if (!any || h > hi) hi = h;
        any = true;
    }
    out->scale = any ? lo : 0; out->bits = any ? (uint32_t)(1 + hi - lo) : 1u; out->nlimbs = (out->bits + 31u) / 32u;
    return out->nlimbs <= (kind == XS_KIND_INT ? 2u : (uint32_t)XS_MAX_LIMBS);
}

// the limbs of raw value v under the column's scale: returns the class, *neg its sign, limb[0 .. XS_MAX_LIMBS) the digits of |v| / 2^scale (zero unless finite).
// A value the scale was computed over shifts out no set bit; digits above the column's nlimbs are zero.
XS_FN uint32_t xs_limbs(uint64_t v, int32_t kind, int32_t scale, uint32_t* neg, uint32_t (&limb)[XS_MAX_LIMBS]) {
    uint64_t mag; int32_t e0;
    const uint32_t cls = xs_unpack(v, kind, neg, &mag, &e0);
    int32_t sh = e0 - scale;                                          // in (-64, 128) for a value of the column; anything else is shifted away, never undefined
    uint64_t lo = 0, hi = 0;
    if (sh <= -64 || sh >= 128) mag = 0;
    if (sh < 0) lo = mag >> (sh <= -64 ? 0 : -sh);
    else if (sh == 0) lo = mag;
    else if (sh < 64) { lo = mag << sh; hi = mag >> (64 - sh); }
    else hi = mag << (sh >= 128 ? 0 : sh - 64);
    if (cls != XS_FINITE) lo = hi = 0;
    limb[0] = (uint32_t)lo; limb[1] = (uint32_t)(lo >> 32); limb[2] = (uint32_t)hi; limb[3] = (uint32_t)(hi >> 32);
    return cls;
}

// ---- the answer, from the limb sums ----
// sum_i S[i] * 2^(32 i) as sign and magnitude
XS_FN XsWide xs_recombine(const int64_t* S, uint32_t nlimbs) {
    uint32_t t[XS_WIDE_WORDS] = {0, 0, 0, 0, 0, 0};                   // two's complement
    for (uint32_t i = 0; i < nlimbs && i < XS_MAX_LIMBS; i++) {
        const uint64_t u = (uint64_t)S[i]; const uint32_t ext = S[i] < 0 ? 0xFFFFFFFFu : 0u;
        uint64_t carry = 0;
        for (uint32_t k = i; k < XS_WIDE_WORDS; k++) {
            const uint32_t add = k == i ? (uint32_t)u : (k == i + 1 ? (uint32_t)(u >> 32) : ext);
            const uint64_t x = (uint64_t)t[k] + add + carry;
            t[k] = (uint32_t)x; carry = x >> 32;
        }
    }
    XsWide W; W.neg = t[XS_WIDE_WORDS - 1] >> 31;
    uint64_t carry = 1; bool any = false;
    for (uint32_t k = 0; k < XS_WIDE_WORDS; k++) {
        uint32_t x = t[k];
        if (W.neg) { const uint64_t y = (uint64_t)(~x) + carry; x = (uint32_t)y; carry = y >> 32; }
        W.w[k] = x; any = any || x;
    }
    if (!any) W.neg = 0;
    return W;
}
// bit `pos` of the nw-word magnitude w (0 beyond it); whether any bit below pos is set
XS_FN uint32_t xs_bit(const uint32_t* w, int32_t nw, int64_t pos) { return pos < 0 || pos >= 32ll * nw ? 0u : (w[pos >> 5] >> (pos & 31)) & 1u; }
XS_FN bool xs_any_below(const uint32_t* w, int32_t nw, int64_t pos) {
    for (int32_t k = 0; k < nw; k++) {
        if (32ll * k >= pos) break;
        const uint32_t m = pos - 32ll * k >= 32 ? 0xFFFFFFFFu : (1u << (pos - 32ll * k)) - 1u;
        if (w[k] & m) return true;
    }
    return false;
}
// (-1)^neg * (w + a fraction in (0, 1) when sticky) * 2^exp2, rounded once to nearest-even, as the bits of a double; beyond the range +-inf
XS_FN uint64_t xs_round(const uint32_t* w, int32_t nw, bool sticky, int64_t exp2, uint32_t neg) {
    int64_t p = -1;
    for (int32_t k = nw - 1; k >= 0 && p < 0; k--) if (w[k]) { int32_t b = 31; while (!((w[k] >> b) & 1u)) b--; p = 32ll * k + b; }
    const uint64_t sign = (uint64_t)(neg & 1u) << 63;
    if (p < 0) return sticky ? sign : 0ull;                           // below every double that is not zero (a zero sum is +0.0)
    const int64_t E = p + exp2;                                       // exponent of the leading bit
    if (E > 1023) return sign | 0x7FF0000000000000ull;
    const int64_t q = E - 52 > -1074 ? E - 52 : -1074;                // exponent of the result's last place (subnormals share -1074)
    const int64_t r = q - exp2;                                       // bits of w below the last place
    uint64_t mant = 0;
    if (r <= 0) { for (int64_t k = p; k >= 0; k--) mant = (mant << 1) | xs_bit(w, nw, k); mant <<= -r; }      // exact: p - r <= 52
    else {
        for (int64_t k = p; k >= r; k--) mant = (mant << 1) | xs_bit(w, nw, k);
        const bool half = xs_bit(w, nw, r - 1) != 0, rest = sticky || xs_any_below(w, nw, r - 1);
        if (half && (rest || (mant & 1ull))) mant++;
    }
    // mant in [0, 2^53]: a normal result has field q + 1075 and mant's bit 52 set, a subnormal field 0 — ((field - 1) << 52) + mant is both, and a
    // mantissa that rounded up to 2^53 (or a subnormal to 2^52) carries into the exponent by itself
    const uint64_t out = ((uint64_t)(q + 1074) << 52) + mant;
    return out >= 0x7FF0000000000000ull ? sign | 0x7FF0000000000000ull : sign | out;
}
// what +inf and -inf members make of a sum or a mean: 0 none of them (the finite answer holds), else the bits of +inf, -inf or a NaN
XS_FN uint64_t xs_inf_answer(uint32_t npinf, uint32_t nninf) {
    return npinf && nninf ? 0x7FF8000000000000ull : npinf ? 0x7FF0000000000000ull : nninf ? 0xFFF0000000000000ull : 0ull;
}
// the bits of the sum of a slot: 2^scale * W rounded once
XS_FN uint64_t xs_sum_bits(const XsWide& W, int32_t scale, uint32_t npinf, uint32_t nninf) {
    if (npinf || nninf) return xs_inf_answer(npinf, nninf);
    return xs_round(W.w, XS_WIDE_WORDS, false, scale, W.neg);
}
// the bits of 2^scale * W / count rounded once (count > 0): W << 96 divided digit by digit, the remainder is the sticky bit
XS_FN uint64_t xs_mean_bits(const XsWide& W, int32_t scale, uint32_t count, uint32_t npinf, uint32_t nninf) {
    if (npinf || nninf) return xs_inf_answer(npinf, nninf);
    uint32_t qd[XS_WIDE_WORDS + XS_QUOT_SHIFT_WORDS];
    uint64_t rem = 0;
    for (int32_t k = XS_WIDE_WORDS + XS_QUOT_SHIFT_WORDS - 1; k >= 0; k--) {
        const uint64_t cur = (rem << 32) | (k >= XS_QUOT_SHIFT_WORDS ? W.w[k - XS_QUOT_SHIFT_WORDS] : 0u);
        qd[k] = (uint32_t)(cur / count); rem = cur % count;
    }
    return xs_round(qd, XS_WIDE_WORDS + XS_QUOT_SHIFT_WORDS, rem != 0, (int64_t)scale - 32 * XS_QUOT_SHIFT_WORDS, W.neg);
}
// the sum of an int column (scale 0) as a 128-bit two's complement integer: fewer than 2^31 values of 64 bits stay inside it
XS_FN void xs_sum_int128(const XsWide& W, uint64_t* lo, int64_t* hi) {
    uint64_t l = (uint64_t)W.w[0] | ((uint64_t)W.w[1] << 32), h = (uint64_t)W.w[2] | ((uint64_t)W.w[3] << 32);
    if (W.neg) { l = ~l + 1ull; h = ~h + (l == 0 ? 1ull : 0ull); }
    *lo = l; *hi = (int64_t)h;
}
