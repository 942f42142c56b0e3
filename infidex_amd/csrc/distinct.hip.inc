// field_distinct: the number of distinct values of a column over the documents a filter accepts, whole and per group (infx_field_distinct).  Included by
// infidex_hip.hip after top_groups.hip.inc.  Not in the reference: exact distinct counts are this project's.
//
// A member's PAIR is (group code, field code), the group code 0 without a group column (distinct_set.h).  A SPEC is (mask, field, group column): its pairs
// are marked in ONE walk over the corpus (set_walk.h, k_field_stats' shape: 16 consecutive documents per thread and step), in one of three placements:
//   k_distinct_lds     G rows of V bits and G size counters in the workgroup's LDS: one LDS OR per member whose bit a plain LDS read shows clear, merged
//                      once — one global atomicOr per word that is not zero, one add per size counter that is not zero
//   k_distinct_bitmap  the rows in global memory (zeroed): a member's atomicOr is issued only when a plain relaxed read of the word shows the bit clear — a
//                      bit is only ever set, so a stale read skips nothing that matters (k_group_heads' trick).  Sizes in LDS counters, merged once
//   k_distinct_hash    the pairs in an open-addressing set of 64-bit keys in global memory (ds_insert: one plain read per slot visited, one compare-and-swap
//                      on an empty one, at most `capacity` slots — then the overflow flag, and the thread stops walking).  The thread whose
//                      compare-and-swap installs a key adds 1 to its group's distinct counter in LDS; sizes likewise; both merged once.  With more than one
//                      group the field code is also marked in a V-bit side row, which gives the whole set's count (chosen over a second key space: the
//                      row costs V / 8 bytes and one read per member once its bits are set; a second key would double the probes of every member)
//   k_distinct_count   placements 1 and 2, and the side row: the popcount of every bitmap word added to its group's counter, one add per wave and row
//   k_distinct_union   more than one row: the rows ORed into a union row, column by column in registers; k_distinct_count of that row is the whole set's
//                      figure.  With one row that row is the whole.
// Only ORs, compare-and-swap installs counted once and integer adds: any grid, stream and placement give the same bytes.  No loop here waits for another
// thread, and every loop has a bound known at its start.
#include "distinct_set.h"
#include "set_walk.h"
#define DST_MAX_REQS 16
#define DST_COUNT_THREADS 256
#define DST_COUNT_GRID 1024                 // k_distinct_count: at most 4096 waves, each with one add per row it meets
#define DST_UNION_ROWS 64u                  // k_distinct_union: rows per thread
#define DST_PLACE_AUTO 0u
#define DST_PLACE_LDS 1u
#define DST_PLACE_BITMAP 2u
#define DST_PLACE_HASH 3u
struct DevDistinct {
    const uint8_t* mask;                    // one byte per document, 0 = in the set; nullptr: every document
    const uint32_t* fcodes;                 // the field
    const uint32_t* gcodes;                 // the group column; nullptr: one group, code 0
    uint32_t* bits;                         // placements 1, 2: gvals rows of rowWords words (zeroed)
    unsigned long long* table;              // placement 3: capacity slots (zeroed)
    uint32_t* side;                         // placement 3 with more than one group: rowWords words (zeroed); else nullptr
    uint32_t* sizes; uint32_t* distinct;    // gvals counters each (zeroed)
    uint32_t* overflow;                     // (zeroed)
    unsigned long long capacity;
    uint32_t gvals, fvals, rowWords, pad;
};

// member(g, v) for every member of the set whose codes are in range; a false return ends the thread's walk
template <class Fn> __device__ __forceinline__ void dst_walk(const DevDistinct& D, int32_t n, Fn member) {
    const uint32_t T = blockDim.x;
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * T + threadIdx.x; g < groups; g += (int64_t)gridDim.x * T) {
        const int64_t d0 = g * LST_GROUP;
        uint32_t m[4], fc[LST_GROUP], gc[LST_GROUP];
        sw_flags16(D.mask, n, d0, m);
        if (!sw_codes16(D.fcodes, n, d0, m, fc)) continue;
        sw_codes16(D.gcodes, n, d0, m, gc);                 // (a null column reads as zeros)
#pragma unroll
        for (int j = 0; j < LST_GROUP; j++) {
            if (!sw_member(m, j) || gc[j] >= D.gvals || fc[j] >= D.fvals) continue;
            if (!member(gc[j], fc[j])) return;
        }
    }
}
// *word |= bit, asked of the memory only when a plain read shows the bit clear
__device__ __forceinline__ void dst_set_lds(uint32_t* word, uint32_t bit) {
    if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) atomicOr(word, bit);
}
__device__ __forceinline__ void dst_set_global(uint32_t* word, uint32_t bits) {
    if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(word, bits);
}
// a member of group g: without a group column into the thread's own counter, else into the group's LDS counter
__device__ __forceinline__ void dst_count_member(const DevDistinct& D, uint32_t* sizes, uint32_t g, uint32_t* mine) {
    if (D.gcodes) atomicAdd(sizes + g, 1u); else ++*mine;
}
// cnt[0 .. k) of the workgroup's LDS into out, one add per counter that is not zero
__device__ __forceinline__ void dst_merge(const uint32_t* cnt, uint32_t* out, uint32_t k) {
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) { const uint32_t x = cnt[i]; if (x) atomicAdd(out + i, x); }
}

// Dynamic LDS: [gvals x rowWords bitmap words | gvals size counters]
__global__ __launch_bounds__(STS_BIG_THREADS) void k_distinct_lds(DevDistinct D, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dst_lds[];
    const uint32_t tid = threadIdx.x, T = blockDim.x, words = D.gvals * D.rowWords;      // STS_THREADS, or STS_BIG_THREADS
    uint32_t* sizes = dst_lds + words;
    for (uint32_t i = tid; i < words + D.gvals; i += T) dst_lds[i] = 0u;
    __syncthreads();
    uint32_t mine = 0;
    dst_walk(D, n, [&](uint32_t g, uint32_t v) {
        dst_set_lds(dst_lds + ds_word(g, D.rowWords, v), ds_bit(v));
        dst_count_member(D, sizes, g, &mine);
        return true;
    });
    if (mine) atomicAdd(sizes, mine);
    __syncthreads();
    for (uint32_t i = tid; i < words; i += T) { const uint32_t x = dst_lds[i]; if (x) atomicOr(D.bits + i, x); }
    dst_merge(sizes, D.sizes, D.gvals);
}

// Dynamic LDS: [gvals size counters]
__global__ __launch_bounds__(STS_THREADS) void k_distinct_bitmap(DevDistinct D, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dst_lds[];
    for (uint32_t i = threadIdx.x; i < D.gvals; i += blockDim.x) dst_lds[i] = 0u;
    __syncthreads();
    uint32_t mine = 0;
    dst_walk(D, n, [&](uint32_t g, uint32_t v) {
        dst_set_global(D.bits + ds_word(g, D.rowWords, v), ds_bit(v));
        dst_count_member(D, dst_lds, g, &mine);
        return true;
    });
    if (mine) atomicAdd(dst_lds, mine);
    __syncthreads();
    dst_merge(dst_lds, D.sizes, D.gvals);
}

// Dynamic LDS: [gvals size counters | gvals distinct counters]
__global__ __launch_bounds__(STS_THREADS) void k_distinct_hash(DevDistinct D, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dst_lds[];
    uint32_t* fresh = dst_lds + D.gvals;
    for (uint32_t i = threadIdx.x; i < 2u * D.gvals; i += blockDim.x) dst_lds[i] = 0u;
    __syncthreads();
    uint32_t mine = 0;
    dst_walk(D, n, [&](uint32_t g, uint32_t v) {
        const int r = ds_insert((uint64_t)D.capacity, ds_key(g, D.fvals, v),
            [&](uint64_t slot) { return (uint64_t)__hip_atomic_load(D.table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
            [&](uint64_t slot, uint64_t key) { return (uint64_t)atomicCAS(D.table + slot, 0ull, (unsigned long long)key); });
        if (r == DS_OVERFLOW) { atomicOr(D.overflow, 1u); return false; }      // the host fails the call
        if (r == DS_NEW) atomicAdd(fresh + g, 1u);
        if (D.side) dst_set_global(D.side + (v >> 5), ds_bit(v));
        dst_count_member(D, dst_lds, g, &mine);
        return true;
    });
    if (mine) atomicAdd(dst_lds, mine);
    __syncthreads();
    dst_merge(dst_lds, D.sizes, D.gvals);
    dst_merge(fresh, D.distinct, D.gvals);
}

// bits: `words` words, rows of rowWords (words < 2^28).  distinct[g] += the bits of row g.  A wave takes a run of whole steps of 64 words and keeps its lanes'
// sums while the steps stay inside one row: one add per wave and row; a step that straddles rows adds lane by lane.
__global__ __launch_bounds__(DST_COUNT_THREADS) void k_distinct_count(const uint32_t* __restrict__ bits, uint32_t words, uint32_t rowWords, uint32_t* __restrict__ distinct) {
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (DST_COUNT_THREADS / 64u) + (threadIdx.x >> 6), waves = gridDim.x * (DST_COUNT_THREADS / 64u);
    const uint32_t per = ((words + waves - 1u) / waves + 63u) & ~63u;
    const uint64_t begin = (uint64_t)wave * per;
    uint32_t cur = 0xFFFFFFFFu, acc = 0;                      // the row the lanes' sums belong to (the same in every lane), none yet
    auto flush = [&]() {
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0 && acc) atomicAdd(distinct + cur, acc);
        acc = 0;
    };
    for (uint32_t k = 0; k < per; k += 64u) {
        if (begin + k >= words) break;                        // (the whole wave)
        const uint32_t w0 = (uint32_t)(begin + k), i = w0 + lane, last = min(w0 + 63u, words - 1u);
        const uint32_t c = i < words ? __popc(bits[i]) : 0u, g0 = w0 / rowWords;
        if (g0 == last / rowWords) {
            if (g0 != cur) { if (cur != 0xFFFFFFFFu) flush(); cur = g0; }
            acc += c;
        } else if (c) atomicAdd(distinct + i / rowWords, c);
    }
    if (cur != 0xFFFFFFFFu) flush();
}

// uni (rowWords words, zeroed) |= the rows [blockIdx.y * chunk, + chunk) of bits: a thread ORs its column of those rows in a register, one atomicOr if any bit is set
__global__ __launch_bounds__(DST_COUNT_THREADS) void k_distinct_union(const uint32_t* __restrict__ bits, uint32_t gvals, uint32_t rowWords, uint32_t chunk, uint32_t* __restrict__ uni) {
    const uint32_t g0 = blockIdx.y * chunk, g1 = min(g0 + chunk, gvals);
    for (uint32_t w = blockIdx.x * DST_COUNT_THREADS + threadIdx.x; w < rowWords; w += gridDim.x * DST_COUNT_THREADS) {
        uint32_t u = 0;
        for (uint32_t g = g0; g < g1; g++) u |= bits[g * rowWords + w];
        if (u) atomicOr(uni + w, u);
    }
}
