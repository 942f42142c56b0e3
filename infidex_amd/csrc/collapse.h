// The arithmetic of Query.collapse_by (k_collapse, collapse.hip.inc): which rows of a ranked list survive "at most `keep` rows per group", where they land and
// how large every group is.  Not in the reference: collapsing is this project's ("collapse_by").
//
// Plain C++ behind CLP_FN, no HIP types: compiled into k_collapse and, unchanged, into a host model that walks the same steps one after the other and holds
// them to a brute-force fold (tests/models/collapse_model.cpp, tests/test_collapse_model.py).
//
// The list L has n rows (n <= CLP_MAX_ROWS), row i in rank order with the group code[i] of its document.  The steps, each a pure function of positions:
//   1. order the row indices by (code, position), the pad indices >= n behind them                                   clp_before
//   2. sorted position p starts a segment when p == 0 or the code before it differs                                  clp_starts
//   3. an exclusive count of the starts in front of p gives p's segment: that count, less one where p starts none    clp_segment
//      seg[g] = the sorted position where segment g starts; seg[groups] = n
//   4. a row's rank in its group is its offset in the segment, the group's size the segment's length                 clp_rank, clp_size
//   5. a row is kept when its rank is below keep                                                                     clp_keeps
//   6. an exclusive count of the kept rows in front of row i, in ROW order, is where row i lands; the first
//      min(kept, mr) of them are written                                                                             clp_returned, clp_emits
// Ranks are positions and counts are integer adds: the order in which a workgroup's threads do the work never shows in the answer.
#pragma once
#include <stdint.h>
#ifndef CLP_FN
#define CLP_FN __host__ __device__ __forceinline__
#endif
#define CLP_MAX_ROWS 1024u                  // rows of a ranked list: CoverageDepth at most
#define CLP_MAX_KEEP 16u                    // rows kept per group (INFX_COLLAPSE_MAX_KEEP)

// (code, position) order of two row indices of a list of n rows; an index >= n is a pad of the power-of-two sort and goes last
CLP_FN bool clp_before(const uint32_t* code, uint32_t n, uint32_t a, uint32_t b) {
    const bool pa = a >= n, pb = b >= n;
    if (pa || pb) return pa != pb ? pb : a < b;
    return code[a] != code[b] ? code[a] < code[b] : a < b;
}
// does sorted position p (< n) start a segment?  idx: the row indices in (code, position) order
template <class Idx> CLP_FN uint32_t clp_starts(const uint32_t* code, const Idx* idx, uint32_t p) { return p == 0 || code[idx[p - 1]] != code[idx[p]] ? 1u : 0u; }
// the segment of sorted position p: `before` starts lie in front of it
CLP_FN uint32_t clp_segment(uint32_t before, uint32_t starts) { return before + starts - 1u; }
template <class Seg> CLP_FN uint32_t clp_rank(const Seg* seg, uint32_t g, uint32_t p) { return p - seg[g]; }
template <class Seg> CLP_FN uint32_t clp_size(const Seg* seg, uint32_t g) { return (uint32_t)seg[g + 1] - (uint32_t)seg[g]; }
CLP_FN uint32_t clp_keeps(uint32_t rank, uint32_t keep) { return rank < keep ? 1u : 0u; }
// rows returned of `kept` kept rows under a budget of mr rows
CLP_FN uint32_t clp_returned(uint32_t kept, uint32_t mr) { return kept < mr ? kept : mr; }
// is row i, kept or not, with `before` kept rows in front of it, one of the `returned` rows?  It lands at `before`.
CLP_FN bool clp_emits(uint32_t keeps, uint32_t before, uint32_t returned) { return keeps && before < returned; }
