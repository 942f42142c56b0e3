// The arithmetic of field_distinct's passes (distinct.hip.inc): where the pair (group code, field code) of a member lies in a bitmap of one row per group,
// and how it enters a hash set of pairs.  Not in the reference: exact distinct counts are this project's ("field_distinct").
//
// Plain C++ behind DS_FN, no HIP types: compiled into k_distinct_lds / k_distinct_bitmap / k_distinct_hash / k_distinct_count and, unchanged, into a host
// model that holds every function to std::set and plain loops under the sanitizers (tests/models/distinct_model.cpp, tests/test_distinct_model.py).
//   pair       (g, v): g the member's code in the group column (0 without one), v its code in the field.  G group values, V field values.
//   bitmap     G rows of V bits, each row padded to whole 32-bit words: ds_row_words(V) words per row.  Pair (g, v) is bit v % 32 of word
//              g * row + v / 32.  A bitmap the device addresses has at most DS_MAX_BITMAP_BITS bits, padding included: a word index fits 32 bits.
//   hash set   open addressing over 64-bit slots, linear probing from ds_hash(key) & (capacity - 1).  The key of a pair is its index g * V + v plus one,
//              0 an empty slot; keys are never removed.  The capacity is the power of two >= 2 x the pairs that can occur — no more than the corpus has
//              documents, no more than G x V — and at least DS_MIN_CAPACITY: the table is never more than half full, so it never fills.
//   insert     ds_insert reads a slot, takes an equal key for "seen", tries ONE compare-and-swap on an empty one and otherwise moves to the next slot.  It
//              visits every slot at most once: after `capacity` slots it gives up with DS_OVERFLOW — no unbounded loop, no waiting for another thread.
//              Exactly one caller is told DS_NEW per key, whatever the interleaving: the one whose compare-and-swap installed it.
#pragma once
#include <stdint.h>
#ifndef DS_FN
#define DS_FN __host__ __device__ __forceinline__
#endif
#define DS_MAX_BITMAP_BITS 0x100000000ull   // 2^32 bits (512 MiB), rows padded
#define DS_MIN_CAPACITY 1024ull             // slots of the smallest hash set
#define DS_SEEN 0                           // ds_insert: the key was there
#define DS_NEW 1                            //            this call installed it
#define DS_OVERFLOW (-1)                    //            every slot visited, the key neither found nor placed

DS_FN uint32_t ds_row_words(uint32_t fvals) { return (uint32_t)(((uint64_t)fvals + 31u) >> 5); }
// the words of a bitmap of G rows (64-bit: the product may exceed what a device bitmap holds; ds_bitmap_fits decides)
DS_FN uint64_t ds_bitmap_words(uint32_t gvals, uint32_t fvals) { return (uint64_t)gvals * ds_row_words(fvals); }
DS_FN bool ds_bitmap_fits(uint32_t gvals, uint32_t fvals) { return ds_bitmap_words(gvals, fvals) * 32u <= DS_MAX_BITMAP_BITS; }
// word and bit of pair (g, v) in a bitmap that fits
DS_FN uint32_t ds_word(uint32_t g, uint32_t rowWords, uint32_t v) { return g * rowWords + (v >> 5); }
DS_FN uint32_t ds_bit(uint32_t v) { return 1u << (v & 31u); }

DS_FN uint64_t ds_pair(uint32_t g, uint32_t fvals, uint32_t v) { return (uint64_t)g * fvals + v; }
DS_FN uint64_t ds_key(uint32_t g, uint32_t fvals, uint32_t v) { return ds_pair(g, fvals, v) + 1u; }
// the pairs a corpus of `docs` documents can hold of G x V
DS_FN uint64_t ds_max_pairs(uint64_t docs, uint32_t gvals, uint32_t fvals) { const uint64_t gv = (uint64_t)gvals * fvals; return docs < gv ? docs : gv; }
// (pairs <= 2^31, the corpus's limit: the capacity is at most 2^32 and the shift cannot run away)
DS_FN uint64_t ds_capacity(uint64_t pairs) { uint64_t c = DS_MIN_CAPACITY; while (c < 2u * pairs && c < (1ull << 62)) c <<= 1; return c; }
// a 64-bit finalizer (MurmurHash3's fmix64): consecutive keys — the codes of one group — spread over the table
DS_FN uint64_t ds_hash(uint64_t key) {
    key ^= key >> 33; key *= 0xFF51AFD7ED558CCDull; key ^= key >> 33; key *= 0xC4CEB9FE1A85EC53ull; key ^= key >> 33;
    return key;
}
// the i-th slot of key's probe sequence in a table of `capacity` slots (a power of two): linear, wrapping at the table's end
DS_FN uint64_t ds_slot(uint64_t key, uint64_t capacity, uint64_t i) { return (ds_hash(key) + i) & (capacity - 1u); }
// key (not 0) into the table.  load(slot) reads a slot; cas(slot, key) stores key where the slot is empty and returns what the slot held before.
template <class Load, class Cas> DS_FN int ds_insert(uint64_t capacity, uint64_t key, Load load, Cas cas) {
    for (uint64_t i = 0; i < capacity; i++) {
        const uint64_t slot = ds_slot(key, capacity, i);
        uint64_t cur = load(slot);
        if (cur == key) return DS_SEEN;
        if (cur == 0) {
            cur = cas(slot, key);
            if (cur == 0) return DS_NEW;
            if (cur == key) return DS_SEEN;
        }
    }
    return DS_OVERFLOW;
}
