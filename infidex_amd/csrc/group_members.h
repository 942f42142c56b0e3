// The arithmetic of list_group_members' walk (group_members.hip.inc): how a member's composite enters the N slots of its group's row, so that the row ends as
// the N smallest composites of the group, ascending.  Not in the reference: the collapsed listing is this project's ("list_group_members").
//
// Plain C++ behind GM_FN, no HIP types: compiled into k_group_members and, unchanged, into a host model that feeds rows from eight threads and holds every
// slot to std::sort (tests/models/group_members_model.cpp, tests/test_group_members_model.py).  The composites are group_heads.h's: (listing key << 32) |
// document, distinct because the document is the low word, never all ones (GH_EMPTY: a slot nothing has entered).
//
// The memory comes from the including file, as a value `mem` with two members:
//   mem.read(j)          a plain (relaxed, untorn) read of slot j
//   mem.take_min(j, v)   slot j <- min(slot j, v) in one step, returning what the slot held before
// The kernels give the 64-bit minimum of the LDS or of global memory, the model a compare-and-swap loop over a std::atomic.
//
// gm_insert(mem, N, comp): v = comp walks the slots 0 .. N-1.  At slot j it asks for the minimum of the slot and v, and carries on what lost: the slot's old
// content where v displaced it, v itself where the slot was smaller.  An empty slot takes v and ends the walk; what is carried past slot N-1 is dropped.
// Where a plain read shows a slot at or below v the minimum is not asked for: a slot only ever decreases, so the minimum would have changed nothing.
//
// Why the slots end right under any interleaving of any number of inserts.  Composites are distinct, and each exists exactly once among the slots, the values
// being carried and the values dropped: a minimum that stores v hands the old content to the same walk, one that does not leaves both where they were.  A value
// that reaches slot j lost at slots 0 .. j-1, so it exceeded their content at that time, and that content only falls afterwards.  A dropped value therefore
// exceeds the final content of all N slots, N distinct composites that were kept: the slots hold the N smallest.  And whatever slot j holds at the end
// came to it past slot j-1 (which was not empty, or the walk had ended there): it exceeds the final content of slot j-1, so the slots ascend, the empty ones
// (all ones) behind.
// The last slot is read before the walk.  What it holds came past slots 0 .. N-2 and exceeded them; they only fall.  So a composite at or above a plain read
// of the last slot is above all N slots as they are now and ever will be: the walk would skip every slot and drop it.  Returning at once is that walk, in
// one read instead of N — the common case for a group with many more members than slots.
// Nothing is sorted or verified after the walk; the model test holds the order.
#pragma once
#include <stdint.h>
#include "group_heads.h"
#ifndef GM_FN
#define GM_FN __host__ __device__ __forceinline__
#endif
#define GM_MAX_PER_GROUP 16u                // members kept per group (INFX_GROUP_MEMBERS_MAX_PER_GROUP)
#define GM_MAX_SLOTS 4096u                  // slots of a request: limit * per_group (INFX_GROUP_MEMBERS_MAX)

// the LDS words of one request in k_group_members: [limit codes | limit counters | limit * per_group slots of two words]; even, so the slots are 8-aligned
GM_FN constexpr uint32_t gm_lds_words(uint32_t limit, uint32_t perGroup) { return 2u * limit + 2u * limit * perGroup; }

template <class Mem> GM_FN void gm_insert(const Mem& mem, uint32_t N, uint64_t comp) {
    uint64_t v = comp;
    if (v >= mem.read(N - 1u)) return;      // the last slot first: the walk below would pass every slot and drop v (above) — one read for most members of a large group
    for (uint32_t j = 0; j < N; j++) {
        if (v >= mem.read(j)) continue;
        const uint64_t old = mem.take_min(j, v);
        if (old == GH_EMPTY) return;
        if (old > v) v = old;
    }
}
