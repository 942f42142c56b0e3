// The arithmetic of range_facets' counting pass (ranges.hip.inc): which counter a document's sort rank goes to, and where a request's thresholds and
// counters lie.  Not in the reference: the buckets are this project's ("range_facets").
//
// Plain C++ behind RB_FN, no HIP types: compiled into k_range_counts and, unchanged, into a host model that walks every rank against a linear scan
// (tests/models/range_model.cpp, tests/test_range_buckets_model.py).
//   edges      e_0 < e_1 < .. < e_B as the column's sort order compares them: B buckets [e_i, e_i+1), all half-open
//   thr[i]     the number of distinct sort ranks of the column whose value compares < e_i (NaN ranks lowest, so it is under every edge): ranks are dense,
//              hence a document of rank r has v >= e_i exactly when thr[i] <= r.  Non-decreasing; equal neighbours are an empty bucket.
//   nanRanks   1 when the column's dictionary holds a NaN (rank 0 then), else 0
//   slot       of rank r: the NaN slot when r < nanRanks, else j = #{i : thr[i] <= r}: 0 below e_0, 1 .. B bucket j - 1, B + 1 at or above e_B
//   counters   per request nedges + 2 = B + 3 words: [below | B buckets | above | nan]; then the smallest and the largest non-NaN rank seen
#pragma once
#include <stdint.h>
#ifndef RB_FN
#define RB_FN __host__ __device__ __forceinline__
#endif
#define RB_MIN_EDGES 2
#define RB_MAX_EDGES 257
#define RB_MAX_REQS 16
#define RB_MAX_SLOTS (RB_MAX_EDGES + 2)     // counters of one request
#define RB_NO_RANK 0xFFFFFFFFu              // a document outside the set; also "no rank yet" of the minimum

// #{i < n : thr[i] <= r} for non-decreasing thr, 1 <= n <= RB_MAX_EDGES: a branch-free upper bound by descending powers of two.  pos is a count already
// known to hold (thr[pos - 1] <= r); a step of size s is taken when pos + s <= n and thr[pos + s - 1] <= r.  The first step is the largest power of two
// <= n, so every count up to n is reachable: floor(log2 n) + 1 reads, nine for 257 thresholds, and the trip count depends on n alone.
RB_FN uint32_t rb_first_step(uint32_t n) { uint32_t s = 1; while ((s << 1) <= n) s <<= 1; return s; }
RB_FN uint32_t rb_upper_bound(const uint32_t* thr, uint32_t n, uint32_t r) {
    uint32_t pos = 0;
    for (uint32_t s = rb_first_step(n); s; s >>= 1) {
        const uint32_t to = pos + s, at = (to <= n ? to : n) - 1u;             // (the read stays inside thr whatever the step)
        pos += (to <= n && thr[at] <= r) ? s : 0u;
    }
    return pos;
}
RB_FN uint32_t rb_slots(uint32_t nedges) { return nedges + 2u; }
RB_FN uint32_t rb_nan_slot(uint32_t nedges) { return nedges + 1u; }
RB_FN uint32_t rb_slot(const uint32_t* thr, uint32_t nedges, uint32_t nanRanks, uint32_t r) {
    const uint32_t j = rb_upper_bound(thr, nedges, r);
    return r < nanRanks ? rb_nan_slot(nedges) : j;
}
// words of a request in the workgroup's LDS: thresholds, counters, min rank, max rank
RB_FN uint32_t rb_lds_words(uint32_t nedges) { return nedges + rb_slots(nedges) + 2u; }
