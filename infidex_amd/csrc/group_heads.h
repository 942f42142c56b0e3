// The arithmetic of list_groups' passes (groups.hip.inc): the number whose minimum over a group is the group's head, and where a member's group code lies
// among the sorted codes of a page.  Not in the reference: the collapsed listing is this project's ("list_groups").
//
// Plain C++ behind GH_FN, no HIP types: compiled into k_group_heads / k_group_heads_mask / k_group_sizes / k_group_members and, unchanged, into a host model that holds the
// lookup to a linear scan and the composite to a comparison of (key, document) pairs (tests/models/group_model.cpp, tests/test_group_model.py).
//   composite  (k << 32) | d: k the member's listing key (listing_select.h: 1 + sort rank, mirrored when descending, 1 without a column), d its document.
//              Composites compare as the listing's order (k, d) does, so the smallest composite of a group is its head — the member that comes first in the
//              listing — and the low word names it.  k >= 1 and d < 2^31: no composite is all ones, the value of an entry no member has touched.
//   page codes the group codes of a page's rows, ascending.  The rows are heads of distinct groups, so the codes are distinct: a member's code is at one
//              position or at none.
#pragma once
#include <stdint.h>
#ifndef GH_FN
#define GH_FN __host__ __device__ __forceinline__
#endif
#define GH_NONE 0xFFFFFFFFu                 // gh_find: the code is not among the page's
#define GH_EMPTY 0xFFFFFFFFFFFFFFFFull      // a head-table entry without a member
#define GH_MAX_CODES 1024u                  // rows of a page (INFX_POST_MAX_ROWS)

GH_FN uint64_t gh_composite(uint32_t key, uint32_t doc) { return ((uint64_t)key << 32) | doc; }
GH_FN uint32_t gh_head(uint64_t entry) { return (uint32_t)entry; }
// document d with composite c is the head of its group exactly when the group's entry is c; the low word decides, since a group's members differ in it
GH_FN bool gh_is_head(uint64_t entry, uint32_t doc) { return entry != GH_EMPTY && gh_head(entry) == doc; }
// The position of `code` among codes[0 .. n), ascending and distinct, 0 <= n <= GH_MAX_CODES; GH_NONE when it is not there.  A branch-free upper bound by
// descending powers of two, as rb_upper_bound (range_buckets.h) but for up to 1024 entries: pos counts the entries known to be <= code, a step of size s is
// taken when pos + s <= n and codes[pos + s - 1] <= code.  The first step is the largest power of two <= n, so every count up to n is reachable:
// floor(log2 n) + 1 reads, eleven for 1024 codes, and the trip count depends on n alone.
GH_FN uint32_t gh_first_step(uint32_t n) { uint32_t s = 1; while ((s << 1) <= n) s <<= 1; return s; }
GH_FN uint32_t gh_find(const uint32_t* codes, uint32_t n, uint32_t code) {
    if (!n) return GH_NONE;
    uint32_t pos = 0;
    for (uint32_t s = gh_first_step(n); s; s >>= 1) {
        const uint32_t to = pos + s, at = (to <= n ? to : n) - 1u;             // (the read stays inside codes whatever the step)
        pos += (to <= n && codes[at] <= code) ? s : 0u;
    }
    return pos && codes[pos - 1u] == code ? pos - 1u : GH_NONE;
}
