// The set walk: how a thread reads the 16 consecutive documents it takes from a document set.  The one reader behind list_documents (listing.hip.inc),
// range_facets (ranges.hip.inc), field_stats (stats.hip.inc), list_groups (groups.hip.inc) and list_group_members (group_members.hip.inc).  Not in the reference: these features are this project's
// ("The set walk").
//
// Plain C++ behind SW_FN, no HIP types: compiled into k_list_hist / k_list_count / k_list_gather / k_range_counts / k_field_stats / k_group_heads /
// k_group_heads_mask / k_group_sizes / k_group_members and, unchanged, into a host model that holds every function to a definition written byte by byte, on heap blocks of
// exactly n elements under the address sanitizer (tests/models/set_walk_model.cpp, tests/test_set_walk_model.py).
//   set        a byte per document, 0 = in the set (a pre-filter mask or the index's Deleted flags); a null pointer: every document.  Neither the flags nor
//              the columns are padded: nothing is read at or beyond n.
//   group      the SW_GROUP documents from d0, a multiple of SW_GROUP; n > 0 and d0 >= 0.  Every launch site walks a corpus of at least one document (the
//              host launches nothing for n = 0); d0 may lie at or beyond n — a thread past the corpus — and then no document is a member.
//   flags      four words: byte j of m[q] is not zero exactly when document d0 + 4q + j is outside the set or the corpus
//   16 bytes   flags and codes of whole groups arrive as ONE 16-byte load each: sw_load16 copies 16 bytes from an address it promises the compiler is
//              16-aligned into a struct of four words, which the device compiles to a single global_load_dwordx4 and the host to a plain copy.  (Chosen
//              over a load function supplied by the including file: the header then reads the same on both sides, and nothing is cast to a vector type.)
#pragma once
#include <stdint.h>
#ifndef SW_FN
#define SW_FN __host__ __device__ __forceinline__
#endif
#define SW_GROUP 16                         // documents per thread and step

struct sw_quad { uint32_t w[4]; };
SW_FN sw_quad sw_load16(const void* p) { sw_quad v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), sizeof v); return v; }

// The flags of the group at d0.  A whole group: one 16-byte load, none for a null mask.  The corpus's partial last group (and a group past the corpus): every
// byte is read at an address clamped into the corpus and every word is built from the values read — no conditional update of m, the form that once
// compiled into a wrong answer ("list_groups", The partial last group).
SW_FN void sw_flags16(const uint8_t* __restrict__ mask, int32_t n, int64_t d0, uint32_t (&m)[4]) {
    if (d0 + SW_GROUP <= (int64_t)n) {
        sw_quad v = {{0, 0, 0, 0}};
        if (mask) v = sw_load16(mask + d0);
        m[0] = v.w[0]; m[1] = v.w[1]; m[2] = v.w[2]; m[3] = v.w[3];
        return;
    }
    uint64_t lo = 0, hi = 0;                // flags 0 .. 7 and 8 .. 15
#pragma nounroll                            // a real loop: unrolled, its 16 clamped addresses are kept in registers across the request loops of k_range_counts / k_field_stats
    for (int j = 0; j < SW_GROUP; j++) {
        const int64_t d = d0 + j;
        const uint32_t flag = mask ? mask[d < (int64_t)n ? d : (int64_t)n - 1] : 0u;
        const uint64_t out = (uint64_t)((d >= (int64_t)n ? 1u : 0u) | (flag ? 1u : 0u)) << (8 * (j & 7));
        lo |= j < 8 ? out : 0; hi |= j < 8 ? 0 : out;
    }
    m[0] = (uint32_t)lo; m[1] = (uint32_t)(lo >> 32); m[2] = (uint32_t)hi; m[3] = (uint32_t)(hi >> 32);
}
// a zero byte in a flag word: a member among its four documents
SW_FN bool sw_any4(uint32_t w) { return ((w - 0x01010101u) & ~w & 0x80808080u) != 0; }
// document d0 + j is a member
SW_FN bool sw_member(const uint32_t (&m)[4], int j) { return !((m[j >> 2] >> (8 * (j & 3))) & 0xFFu); }
// The codes of the group's documents in column col, m its flags; false: no member among the 16.  A four without a member is not loaded and reads as zeros,
// and so does every four of a null column.  A whole four is one 16-byte load; the corpus's last, partial four is read element by element, below n only.
SW_FN bool sw_codes16(const uint32_t* __restrict__ col, int32_t n, int64_t d0, const uint32_t (&m)[4], uint32_t (&cc)[SW_GROUP]) {
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const bool some = sw_any4(m[q]);
        sw_quad c = {{0, 0, 0, 0}};
        if (some && col) {
            const int64_t dq = d0 + 4 * q;
            if (dq + 4 <= (int64_t)n) c = sw_load16(col + dq);
            else { if (dq < n) c.w[0] = col[dq]; if (dq + 1 < n) c.w[1] = col[dq + 1]; if (dq + 2 < n) c.w[2] = col[dq + 2]; }
        }
        cc[4 * q] = c.w[0]; cc[4 * q + 1] = c.w[1]; cc[4 * q + 2] = c.w[2]; cc[4 * q + 3] = c.w[3];
        any = any || some;
    }
    return any;
}
