// The arithmetic of field_quantiles' selection (quantiles.hip.inc): the key at position floor((count - 1) * q) of the non-NaN members of a SLOT (one group
// code of one request, or the whole set), for up to QS_MAX_Q quantiles of every slot of every request at once.  A radix select over the keys, most
// significant digit first; the digit arithmetic is listing_select.h's (ls_passes, ls_shift, ls_digit, ls_under_prefix, ls_extend, ls_pick), reused here.
// Not in the reference: the quantiles are this project's ("field_quantiles").
//
// Plain C++ behind LS_FN, no HIP types: compiled into k_quant_hist / k_quant_pick and, unchanged, into a host model that walks the whole select serially and
// compares every target with a plain sort (tests/models/quantile_model.cpp, tests/test_quantile_model.py).
//   key        k = 1 + sort rank of the member's value: 1 .. nvals; a member whose rank is below nan_ranks is a NaN: counted, in no quantile
//   target     one (slot, quantile): {prefix, resid} as an ls_target; prefix = QS_DEAD: the slot has no non-NaN member
//   pass 0     every target of a slot is under the empty prefix: ONE row of 2^w bins per slot plus a NaN counter (qs_row0 words); the row's sum is the
//              slot's count, which turns every q into its position (qs_position) and the position into the first digit
//   pass p     one row of 2^w bins per target: the members of the slot whose higher digits equal the target's prefix
//   answer     after the last pass prefix is the key: the value's sort rank is prefix - 1
#pragma once
#include "listing_select.h"
#define QS_MAX_Q 16
#define QS_DEAD 0xFFFFFFFFu                 // no key reaches it: keys are ranks + 1 of fewer than 2^31 documents

// words of a slot's row in pass 0: the bins and the NaN counter behind them
LS_FN uint32_t qs_row0(uint32_t digitBits) { return (1u << digitBits) + 1u; }
// words of a slot in a pass: one row in pass 0, a row per quantile later
LS_FN uint32_t qs_slot_words(uint32_t pass, uint32_t nq, uint32_t digitBits) { return pass ? nq << digitBits : qs_row0(digitBits); }
// The 0-based position of quantile q (0 <= q <= 1) among count >= 1 ordered members: floor((count - 1) * q), the product ONE IEEE double multiplication — what
// numpy.quantile(method="lower") picks.  count - 1 < 2^31 is exact as a double and the product is not negative: the conversion truncates, which is the floor.
LS_FN uint32_t qs_position(uint32_t count, double q) { const double x = (double)(count - 1u) * q; return (uint32_t)x; }
// the key of a member of sort rank r; 0: a NaN
LS_FN uint32_t qs_key(uint32_t r, uint32_t nanRanks) { return r < nanRanks ? 0u : r + 1u; }
// A target before pass 0: the empty prefix and the quantile's position among the slot's count non-NaN members; dead without one
LS_FN ls_target qs_start(uint32_t count, double q) { ls_target t; t.prefix = count ? 0u : QS_DEAD; t.resid = count ? qs_position(count, q) : 0u; return t; }
// One digit more for target cur from PART of its row of this pass: part holds bins [b0, b0 + nb) of the row, excl is the sum of the bins before b0 (the
// whole row: b0 = 0, excl = 0; k_quant_pick gives every lane of a wave a part).  true: the target's position lies in this part, *out is the target under its
// longer prefix.  Exactly one part of a row answers true while the target is alive and the row holds its position.
LS_FN bool qs_step(ls_target cur, const uint32_t* part, uint32_t b0, uint32_t nb, uint32_t excl, uint32_t digitBits, ls_target* out) {
    if (cur.prefix == QS_DEAD || cur.resid < excl) return false;
    uint32_t dg = 0, rest = 0;
    if (!ls_pick(part, nb, cur.resid - excl, &dg, &rest)) return false;
    out->prefix = ls_extend(cur.prefix, b0 + dg, digitBits); out->resid = rest;
    return true;
}
// the sort rank a resolved target answers with (QS_DEAD: none)
LS_FN uint32_t qs_rank(ls_target t) { return t.prefix == QS_DEAD ? QS_DEAD : t.prefix - 1u; }
// The smallest digit width that needs no more passes than w does for nvals values: the same launches, smaller tables.
LS_FN uint32_t qs_narrow(uint32_t nvals, uint32_t w) {
    const uint32_t p = ls_passes(nvals, w);
    while (w > LS_MIN_DIGIT_BITS && ls_passes(nvals, w - 1u) == p) w--;
    return w;
}
