// The arithmetic of list_documents' selection (listing.hip.inc): positions [offset, offset + limit) of a document set in the order (key, document) are
// found by a radix select over the keys, most significant digit first, for TWO positions at once (the page's first and last), then the page is cut out
// of the three key classes the two thresholds leave.  Not in the reference: the order and the paging are this project's ("list_documents").
//
// Plain C++ behind LS_FN, no HIP types: compiled into k_list_hist / k_list_pick / k_list_count / k_list_gather and, unchanged, into a host model that walks
// the whole select serially and compares it with a plain sort (tests/models/listing_model.cpp, tests/test_listing_model.py).
//   key        k(d) = 1 + rank of the document's value (ascending), or its mirror nvals + 1 - k (descending): 1 .. nvals either way, 0 is no key
//   pass p     of P = ceil(B / w) passes (B = bits of nvals + 1, w = digit_bits): digit = (k >> (P - 1 - p) * w) & (2^w - 1), counted for the documents
//              whose higher digits equal the target's prefix
//   target     {prefix: the digits chosen so far, resid: the target's position among the documents under that prefix}; after the last pass prefix is the
//              threshold key T and resid the position among the documents of key T in document order (the tie index), so below = position - resid
//   page       class 1: k == T_lo, class 2: T_lo < k < T_hi, class 3: k == T_hi (T_lo < T_hi); a document's slot follows from its index inside its class
#pragma once
#include <stdint.h>
#ifndef LS_FN
#define LS_FN __host__ __device__ __forceinline__
#endif
#define LS_MIN_DIGIT_BITS 4
#define LS_MAX_DIGIT_BITS 11
#define LS_MAX_BINS (1u << LS_MAX_DIGIT_BITS)
#define LS_NONE 0xFFFFFFFFu

struct ls_target { uint32_t prefix, resid; };
// what the select leaves for the gather: thresholds, the first wanted tie index at T_lo, the last wanted tie index at T_hi, rows of the page
struct ls_page { uint32_t tLo, tHi, tieLo, tieHi, count; };

// descending order is ascending order of the mirrored key; ties stay in document order in both
LS_FN uint32_t ls_mirror(uint32_t k, uint32_t nvals, bool ascending) { return ascending ? k : (uint32_t)((uint64_t)nvals + 1u - k); }
// the listing key of a member whose value has dictionary code `code`: 1 + rank[code] (0 for a code beyond the table), mirrored when descending; 1 without a
// column (rank == nullptr: document order)
LS_FN uint32_t ls_key(const uint32_t* rank, uint32_t code, uint32_t nvals, bool ascending) {
    return rank ? ls_mirror(1u + (code < nvals ? rank[code] : 0u), nvals, ascending) : 1u;
}
// B: the bits of nvals + 1 (keys are 1 .. nvals)
LS_FN uint32_t ls_key_bits(uint32_t nvals) { uint32_t b = 0; for (uint64_t v = (uint64_t)nvals + 1u; v; v >>= 1) b++; return b; }
LS_FN uint32_t ls_passes(uint32_t nvals, uint32_t digitBits) { return (ls_key_bits(nvals) + digitBits - 1) / digitBits; }
LS_FN uint32_t ls_shift(uint32_t pass, uint32_t passes, uint32_t digitBits) { return (passes - 1 - pass) * digitBits; }
LS_FN uint32_t ls_digit(uint32_t k, uint32_t shift, uint32_t digitBits) { return (uint32_t)((uint64_t)k >> shift) & ((1u << digitBits) - 1u); }
// the digits of k above the current one equal the target's prefix (shift + digitBits may reach 33: 64-bit shift)
LS_FN bool ls_under_prefix(uint32_t k, uint32_t prefix, uint32_t shift, uint32_t digitBits) { return (uint32_t)((uint64_t)k >> (shift + digitBits)) == prefix; }
LS_FN uint32_t ls_extend(uint32_t prefix, uint32_t digit, uint32_t digitBits) { return (uint32_t)(((uint64_t)prefix << digitBits) | digit); }
// The digit that holds position resid of a histogram: the first bin b with hist[0] + .. + hist[b] > resid; *rest = resid - (hist[0] + .. + hist[b - 1]).
// false: the histogram holds no more than resid entries.
LS_FN bool ls_pick(const uint32_t* hist, uint32_t nbins, uint32_t resid, uint32_t* digit, uint32_t* rest) {
    uint32_t run = 0;
    for (uint32_t b = 0; b < nbins; b++) {
        const uint32_t h = hist[b];
        if (resid - run < h) { *digit = b; *rest = resid - run; return true; }      // (run <= resid always)
        run += h;
    }
    return false;
}
// The page of positions [offset, last] (last >= offset) once both targets are resolved: lo.prefix / hi.prefix are the keys at the two positions, lo.resid /
// hi.resid their tie indices.
LS_FN ls_page ls_make_page(ls_target lo, ls_target hi, uint32_t offset, uint32_t last) {
    ls_page P; P.tLo = lo.prefix; P.tHi = hi.prefix; P.tieLo = lo.resid; P.tieHi = hi.resid; P.count = last - offset + 1u;
    return P;
}
// 0: not on the page whatever its tie index; 1: k == T_lo (the only class when T_lo == T_hi); 2: strictly between; 3: k == T_hi
LS_FN uint32_t ls_class(const ls_page& P, uint32_t k) {
    if (!P.count || k < P.tLo || k > P.tHi) return 0u;
    if (k == P.tLo) return 1u;
    return k == P.tHi ? 3u : 2u;
}
// Slot (0 .. count - 1) of the document that is number idx, in document order, among the set's documents of class cls; LS_NONE when it is off the page.
// eqLo: how many documents of the set carry key T_lo.  The slots of the three classes follow one another, so each is written exactly once.
LS_FN uint32_t ls_slot(const ls_page& P, uint32_t cls, uint32_t idx, uint32_t eqLo) {
    if (cls == 1u) {
        if (idx < P.tieLo || (P.tLo == P.tHi && idx > P.tieHi)) return LS_NONE;
        return idx - P.tieLo;
    }
    if (cls == 2u) return eqLo - P.tieLo + idx;
    if (cls == 3u) return idx <= P.tieHi ? P.count - 1u - P.tieHi + idx : LS_NONE;
    return LS_NONE;
}
