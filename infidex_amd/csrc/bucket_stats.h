// The arithmetic of bucket_stats' pass (bucket_stats.hip.inc): which slot a member's value is added to — the slot of the range bucket its bucket column's sort
// rank falls in — what it adds there, and where a request's thresholds and slots lie.  Not in the reference: the aggregate is this project's (DESIGN.md,
// "bucket_stats").
//
// Plain C++ behind BKS_FN, no HIP types: compiled into k_bucket_stats and, unchanged, into a host model that holds every slot to a brute-force scan
// (tests/models/bucket_stats_model.cpp, tests/test_bucket_stats_model.py).  The bucket lookup is range_buckets.h's rb_slot and the limbs are exact_sum.h's
// xs_limbs; neither is restated here.
//   slots      per request rb_slots(nedges) = B + 3, in rb_slot's order [below | B buckets | above | nan]: bks_slots
//   slot       BKS_HEAD + 2 L words, field_stats' slot (stats.hip.inc): four counters by class (finite, NaN, +inf, -inf), the largest non-NaN sort rank of
//              the VALUE column, a word for the smallest (kept there while the slot lies in LDS), L signed 64-bit limb sums
//   LDS        a call's thresholds first — every request's, always, BKS_MAX_THR_WORDS at the most — then the slots of the requests placed there
//   member     (bucket rank, thresholds, nanRanks) -> the slot; the raw value -> class, sign and limbs: bks_member
#pragma once
#include "range_buckets.h"
#include "exact_sum.h"
#ifndef BKS_FN
#define BKS_FN __host__ __device__ __forceinline__
#endif
#define BKS_MAX_REQS RB_MAX_REQS
#define BKS_HEAD 6u                                              // words of a slot in front of its limb sums (stats.hip.inc's STS_HEAD)
#define BKS_MAX_THR_WORDS (BKS_MAX_REQS * (RB_MAX_EDGES + 3u))   // sixteen requests of 257 thresholds, each rounded up to four words

BKS_FN uint32_t bks_stride(uint32_t nlimbs) { return BKS_HEAD + 2u * nlimbs; }
BKS_FN uint32_t bks_slots(uint32_t nedges) { return rb_slots(nedges); }
BKS_FN uint32_t bks_slot_words(uint32_t nedges, uint32_t nlimbs) { return bks_slots(nedges) * bks_stride(nlimbs); }
// the words a request's thresholds take in LDS: rounded up to four, so that every request's thresholds and the slots behind them start on 16 bytes
BKS_FN uint32_t bks_thr_words(uint32_t nedges) { return (nedges + 3u) & ~3u; }
// the LDS words of a request whose slots lie there too
BKS_FN uint32_t bks_lds_words(uint32_t nedges, uint32_t nlimbs) { return bks_thr_words(nedges) + bks_slot_words(nedges, nlimbs); }

// what one member adds: to slot `slot` of its request one count of class cls, rank (RB_NO_RANK for a NaN: none) to the extreme ranks, +-limb[i] to sum i
struct BksMember { uint32_t slot, cls, neg, rank; uint32_t limb[XS_MAX_LIMBS]; };
// The member whose bucket column has sort rank brank (over thr[0 .. nedges) and nanRanks, range_buckets.h) and whose value column has raw value v of sort
// rank vrank (kind and scale: the value column's, exact_sum.h)
BKS_FN BksMember bks_member(const uint32_t* thr, uint32_t nedges, uint32_t nanRanks, uint32_t brank, uint64_t v, uint32_t vrank, int32_t kind, int32_t scale) {
    BksMember M;
    M.slot = rb_slot(thr, nedges, nanRanks, brank);
    M.cls = xs_limbs(v, kind, scale, &M.neg, M.limb);
    M.rank = M.cls != XS_NAN ? vrank : RB_NO_RANK;
    return M;
}
