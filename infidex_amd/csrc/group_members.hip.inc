// list_group_members: list_groups' page with the first per_group members of every listed group, in list_documents' order (infx_list_group_members).  Included
// by infidex_hip.hip after groups.hip.inc, whose head pass, heads mask, page select and k_group_page are the front half of the call.  Not in the reference:
// the collapsed listing is this project's.
//   k_group_members      takes k_group_sizes' place: ONE walk over the SET for the requests of a spec that fit the LDS together.  Per request the workgroup's
//                        LDS holds the page's sorted codes, one counter per row and limit * per_group slots of 8 bytes, all ones.  A member's group code is
//                        looked up branch-free (gh_find); a hit adds to the row's counter and enters its composite (group_heads.h) into the row's slots
//                        with gm_insert (group_members.h): the slots end as the row's per_group smallest composites, ascending.  The order column is read
//                        for hits only.  At the end every LDS slot that is not empty enters the row's global slots with the same gm_insert, and every
//                        counter that is not zero takes one global add.
//   k_group_member_rows  one workgroup per request: per (row, place) the member's document (-1: none), its DocumentKey and its code of the order column;
//                        per row the slots that are not empty.
// Minima and integer adds only, and gm_insert's result does not depend on the interleaving: any grid, stream and packing give the same bytes.
#include "group_members.h"
#define GM_STATIC_LDS_WORDS INFX_MAX_PREFILTERS                           // k_group_members' own LDS beside the requests': the pages' row counts
#define GM_PACK_LDS_WORDS (GRP_BIG_LDS_WORDS - GM_STATIC_LDS_WORDS)        // what the requests of one launch may take together: the rest of a CU's LDS
struct DevGroupMembers {
    const uint8_t* mask; const uint32_t* gcodes;
    const uint32_t* ocodes; const uint32_t* orank;      // the ordered column and its sort rank; nullptr: constant key (document order)
    uint32_t gvals, onvals, ascending, nreq;
    const uint32_t* cnt[INFX_MAX_PREFILTERS];           // rows of request q's page
    const uint32_t* sorted[INFX_MAX_PREFILTERS];        // their group codes, ascending
    const uint32_t* perm[INFX_MAX_PREFILTERS];          // the row of each
    uint32_t* sizes[INFX_MAX_PREFILTERS];               // per row (zeroed)
    unsigned long long* slots[INFX_MAX_PREFILTERS];     // per row perGroup slots (all ones)
    uint32_t ldsOff[INFX_MAX_PREFILTERS], limit[INFX_MAX_PREFILTERS], perGroup[INFX_MAX_PREFILTERS];      // request q's LDS words (gm_lds_words) from ldsOff
};
// gm_insert's memory: a row's slots in the workgroup's LDS, or in global memory (two types: the address space is the pointer's origin)
struct GmLdsSlots {
    unsigned long long* s;
    __device__ __forceinline__ uint64_t read(uint32_t j) const { return __hip_atomic_load(s + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ uint64_t take_min(uint32_t j, uint64_t v) const { return atomicMin(s + j, (unsigned long long)v); }
};
struct GmGlobalSlots {
    unsigned long long* s;
    __device__ __forceinline__ uint64_t read(uint32_t j) const { return __hip_atomic_load(s + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint64_t take_min(uint32_t j, uint64_t v) const { return atomicMin(s + j, (unsigned long long)v); }
};

// Dynamic LDS: per request its limit codes, limit counters and limit * perGroup slots.
__global__ __launch_bounds__(GRP_BIG_THREADS) void k_group_members(DevGroupMembers Z, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t gm_lds[];
    __shared__ uint32_t rows[INFX_MAX_PREFILTERS];
    const int tid = threadIdx.x; const uint32_t T = blockDim.x;
    if (tid < (int)Z.nreq) rows[tid] = min(*Z.cnt[tid], Z.limit[tid]);
    __syncthreads();
    for (uint32_t q = 0; q < Z.nreq; q++) {
        uint32_t* L = gm_lds + Z.ldsOff[q]; const uint32_t r = rows[q], lim = Z.limit[q];
        unsigned long long* S = (unsigned long long*)(L + 2u * lim);
        for (uint32_t i = tid; i < r; i += T) { L[i] = Z.sorted[q][i]; L[lim + i] = 0u; }
        for (uint32_t i = tid; i < r * Z.perGroup[q]; i += T) S[i] = GH_EMPTY;
    }
    __syncthreads();
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * T + tid; g < groups; g += (int64_t)gridDim.x * T) {
        const int64_t d0 = g * LST_GROUP;
        uint32_t m[4], gc[LST_GROUP];
        sw_flags16(Z.mask, n, d0, m);
        if (!sw_codes16(Z.gcodes, n, d0, m, gc)) continue;
        for (uint32_t q = 0; q < Z.nreq; q++) {
            const uint32_t r = rows[q];
            if (!r) continue;
            uint32_t* L = gm_lds + Z.ldsOff[q]; const uint32_t lim = Z.limit[q], pg = Z.perGroup[q];
            unsigned long long* S = (unsigned long long*)(L + 2u * lim);
#pragma unroll
            for (int j = 0; j < LST_GROUP; j++) {
                if (!sw_member(m, j) || gc[j] >= Z.gvals) continue;
                const uint32_t pos = gh_find(L, r, gc[j]);
                if (pos == GH_NONE) continue;
                atomicAdd(L + lim + pos, 1u);
                const uint32_t oc = Z.ocodes ? Z.ocodes[d0 + j] : 0u;      // (a member: d0 + j < n)
                gm_insert(GmLdsSlots{S + pos * pg}, pg, gh_composite(ls_key(Z.orank, oc, Z.onvals, Z.ascending != 0), (uint32_t)(d0 + j)));
            }
        }
    }
    __syncthreads();
    for (uint32_t q = 0; q < Z.nreq; q++) {
        const uint32_t* L = gm_lds + Z.ldsOff[q]; const uint32_t r = rows[q], lim = Z.limit[q], pg = Z.perGroup[q];
        const unsigned long long* S = (const unsigned long long*)(L + 2u * lim);
        for (uint32_t i = tid; i < r; i += T) { const uint32_t x = L[lim + i]; if (x) atomicAdd(Z.sizes[q] + Z.perm[q][i], x); }
        for (uint32_t i = tid; i < r * pg; i += T) {
            const unsigned long long v = S[i];
            if (v != GH_EMPTY) gm_insert(GmGlobalSlots{Z.slots[q] + (size_t)Z.perm[q][i / pg] * pg}, pg, v);
        }
    }
}

// grid: the spec's requests (ocodes: the spec's order column), each with INFX_GROUP_MEMBERS_MAX slots and places and INFX_POST_MAX_ROWS member counts.  Every
// place of the request's limit * perGroup is written: a slot nothing entered reads -1 / -1 / 0.
struct DevMemberRows { uint32_t limit[INFX_MAX_PREFILTERS], perGroup[INFX_MAX_PREFILTERS]; };
__global__ __launch_bounds__(LST_SORT_THREADS) void k_group_member_rows(const unsigned long long* __restrict__ slots0, DevMemberRows W, const uint32_t* __restrict__ ocodes, int32_t n,
                                                                         const long long* __restrict__ docKeyAll, long long* __restrict__ keys0, int32_t* __restrict__ docs0,
                                                                         uint32_t* __restrict__ codes0, uint32_t* __restrict__ held0) {
    const uint32_t q = blockIdx.x, lim = min(W.limit[q], (uint32_t)INFX_POST_MAX_ROWS), pg = min(W.perGroup[q], GM_MAX_PER_GROUP);
    const uint32_t places = min(lim * pg, GM_MAX_SLOTS);
    const size_t at = (size_t)q * GM_MAX_SLOTS;
    for (uint32_t i = threadIdx.x; i < places; i += LST_SORT_THREADS) {
        const unsigned long long v = slots0[at + i];
        const uint32_t d = (uint32_t)v;
        const bool ok = v != GH_EMPTY && d < (uint32_t)n;
        keys0[at + i] = ok ? docKeyAll[d] : -1; docs0[at + i] = ok ? (int32_t)d : -1; codes0[at + i] = ok && ocodes ? ocodes[d] : 0u;
    }
    for (uint32_t r = threadIdx.x; r < lim; r += LST_SORT_THREADS) {
        uint32_t c = 0;
        for (uint32_t p = 0; p < pg; p++) { const uint32_t i = r * pg + p; c += i < places && slots0[at + i] != GH_EMPTY ? 1u : 0u; }
        held0[(size_t)q * INFX_POST_MAX_ROWS + r] = c;
    }
}
