// list_groups: one row per value of a group column over the documents a filter accepts — the group's head, the member that comes first in list_documents'
// order — by page, with the size of every listed group (infx_list_grouped).  Included by infidex_hip.hip after stats.hip.inc.  Not in the reference: the
// collapsed listing is this project's.
//
// The set is a byte per document, 0 = in the set, as in listing.hip.inc.  A SPEC is (mask, group column, order column, direction): its heads are found once,
// whatever the pages asked of it.  A member's composite is (listing key << 32) | document (group_heads.h): the head of a group is its smallest composite.
//   k_group_heads       ONE walk over the corpus, k_field_stats' shape: a thread takes 16 consecutive documents (set_walk.h).  The head table holds 8 B per value of the group column, all ones = no member: a member takes the 64-bit
//                       minimum of its composite into the entry of its group code, and only when the composite is below what a plain read of the entry
//                       shows — the entry only ever decreases, so a stale read skips no update that matters.  Tables that fit lie in LDS per workgroup
//                       (GRP_LDS_WORDS under 256 threads, else GRP_BIG_LDS_WORDS under one workgroup of 1024 per CU) and are merged once, one global
//                       atomicMin per entry that saw a member; larger ones are hit in global memory.  The walk also counts the members (the set's size).
//   k_group_heads_mask  the heads as a mask slot: byte d is 0 exactly when d is a member and the low word of its group's entry is d; 16 bytes per store.
//                       listing.hip.inc's select / gather / sort then page over that mask unchanged: its total is the number of groups with a member.
//   k_group_page        one workgroup per request of the spec: the group codes of the page's rows, and the same codes sorted ascending with the row each
//                       came from (bitonic in LDS).  The rows' sizes are zeroed here.
//   k_group_sizes       ONE further walk over the SET for all requests of the spec: per workgroup the sorted codes and one counter per row lie in LDS, a
//                       member's group code is looked up branch-free (gh_find) and a hit adds to the row's LDS counter; one global add per counter that is
//                       not zero at the end.
// A minimum has no order and the adds are integer adds: any grid, stream and placement give the same bytes.  No atomic decides a position.
#include "group_heads.h"
#include "set_walk.h"
#define GRP_THREADS 256
#define GRP_BIG_THREADS 1024                // with GRP_BIG_LDS_WORDS: one workgroup per CU, the same sixteen waves
#define GRP_LDS_WORDS STS_LDS_WORDS         // k_field_stats' two budgets
#define GRP_BIG_LDS_WORDS STS_BIG_LDS_WORDS
struct DevGroupSpec {
    const uint8_t* mask;                    // one byte per document, 0 = in the set; nullptr: every document
    const uint32_t* gcodes;                 // the group column
    const uint32_t* ocodes; const uint32_t* orank;      // the ordered column and its sort rank; nullptr: constant key (document order)
    unsigned long long* table;              // gvals entries (all ones)
    uint8_t* heads;                         // the heads mask: the corpus rounded up to whole groups of 16 bytes
    uint32_t* total;                        // the set's size (zeroed)
    uint32_t gvals, onvals, ascending, inLds;
};
struct DevGroupSizes {
    const uint8_t* mask; const uint32_t* gcodes;
    uint32_t nreq, pad;
    const uint32_t* cnt[INFX_MAX_PREFILTERS];           // rows of request q's page
    const uint32_t* sorted[INFX_MAX_PREFILTERS];        // their group codes, ascending
    const uint32_t* perm[INFX_MAX_PREFILTERS];          // the row of each
    uint32_t* sizes[INFX_MAX_PREFILTERS];               // per row (zeroed)
    uint32_t ldsOff[INFX_MAX_PREFILTERS], limit[INFX_MAX_PREFILTERS];      // request q's LDS words: [limit codes | limit counters] from ldsOff
};
// entry <- min(entry, comp), asked of the memory only when a plain read shows a larger entry (one aligned 8-byte load: it is never torn)
__device__ __forceinline__ void grp_take_min(unsigned long long* entry, unsigned long long comp) {
    if (comp < __hip_atomic_load(entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(entry, comp);
}

// G.table all ones, *G.total zero.  Dynamic LDS: G.gvals entries when G.inLds, then (always) the workgroup's member counter.
__global__ __launch_bounds__(GRP_BIG_THREADS) void k_group_heads(DevGroupSpec G, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long grp_tab[];
    const int tid = threadIdx.x; const uint32_t T = blockDim.x;      // GRP_THREADS, or GRP_BIG_THREADS
    uint32_t* members = (uint32_t*)(grp_tab + (G.inLds ? G.gvals : 0u));
    if (G.inLds) for (uint32_t i = tid; i < G.gvals; i += T) grp_tab[i] = GH_EMPTY;
    if (tid == 0) *members = 0;
    __syncthreads();
    uint32_t mine = 0;
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * T + tid; g < groups; g += (int64_t)gridDim.x * T) {
        const int64_t d0 = g * LST_GROUP;
        uint32_t m[4], gc[LST_GROUP], oc[LST_GROUP];
        sw_flags16(G.mask, n, d0, m);
        if (!sw_codes16(G.gcodes, n, d0, m, gc)) continue;
        sw_codes16(G.ocodes, n, d0, m, oc);
#pragma unroll
        for (int j = 0; j < LST_GROUP; j++) {
            if (!sw_member(m, j)) continue;
            mine++;
            if (gc[j] >= G.gvals) continue;
            const unsigned long long comp = gh_composite(ls_key(G.orank, oc[j], G.onvals, G.ascending != 0), (uint32_t)(d0 + j));
            if (G.inLds) grp_take_min(grp_tab + gc[j], comp); else grp_take_min(G.table + gc[j], comp);      // (two inlined copies: ds_min_u64 / global_atomic_umin_x2)
        }
    }
    if (mine) atomicAdd(members, mine);
    __syncthreads();
    if (tid == 0 && *members) atomicAdd(G.total, *members);
    if (G.inLds) for (uint32_t i = tid; i < G.gvals; i += T) { const unsigned long long v = grp_tab[i]; if (v != GH_EMPTY) grp_take_min(G.table + i, v); }
}

// byte d of G.heads: 0 = d is the head of its group.  Every group of 16 bytes up to the corpus rounded up is written, each once.
__global__ __launch_bounds__(GRP_THREADS) void k_group_heads_mask(DevGroupSpec G, int32_t n) {
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * GRP_THREADS) {
        const int64_t d0 = g * LST_GROUP;
        uint32_t m[4], gc[LST_GROUP], out[4] = {0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
        sw_flags16(G.mask, n, d0, m);
        if (sw_codes16(G.gcodes, n, d0, m, gc)) {
#pragma unroll
            for (int j = 0; j < LST_GROUP; j++) {
                if (!sw_member(m, j) || gc[j] >= G.gvals) continue;
                if (gh_is_head(G.table[gc[j]], (uint32_t)(d0 + j))) out[j >> 2] &= ~(0xFFu << (8 * (j & 3)));
            }
        }
        *(uint4*)(G.heads + d0) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// grid: the spec's requests.  docs / cnt: the page k_list_sort left; gout: the rows' group codes; sorted / perm: the codes ascending and the row of each
__global__ __launch_bounds__(LST_SORT_THREADS) void k_group_page(const uint32_t* __restrict__ gcodes, int32_t n, const int32_t* __restrict__ docs0, const uint32_t* __restrict__ cnt0,
                                                                  uint32_t* __restrict__ gout0, uint32_t* __restrict__ sorted0, uint32_t* __restrict__ perm0, uint32_t* __restrict__ sizes0) {
    __shared__ unsigned long long v[INFX_POST_MAX_ROWS];
    const uint32_t i = threadIdx.x; const size_t at = (size_t)blockIdx.x * INFX_POST_MAX_ROWS;
    const uint32_t nrow = min(cnt0[blockIdx.x], (uint32_t)INFX_POST_MAX_ROWS);
    uint32_t c = 0xFFFFFFFFu;
    if (i < nrow) { const int32_t d = docs0[at + i]; if (d >= 0 && d < n) c = gcodes[d]; }
    gout0[at + i] = i < nrow ? c : 0u; sizes0[at + i] = 0u;
    if (!nrow) return;
    uint32_t m = 2; while (m < nrow) m <<= 1;                               // the sorted length: a power of two, padded with the largest composite
    v[i] = i < nrow ? ((unsigned long long)c << 32) | i : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t x = i ^ j;
            if (i < m && x > i) {
                const unsigned long long a = v[i], b = v[x];
                if ((a > b) == ((i & k) == 0)) { v[i] = b; v[x] = a; }
            }
            __syncthreads();
        }
    if (i < nrow) { sorted0[at + i] = (uint32_t)(v[i] >> 32); perm0[at + i] = (uint32_t)v[i]; }
}

// Dynamic LDS: per request its limit codes and limit counters.
__global__ __launch_bounds__(GRP_BIG_THREADS) void k_group_sizes(DevGroupSizes Z, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t grp_lds[];
    __shared__ uint32_t rows[INFX_MAX_PREFILTERS];
    const int tid = threadIdx.x; const uint32_t T = blockDim.x;
    if (tid < (int)Z.nreq) rows[tid] = min(*Z.cnt[tid], Z.limit[tid]);
    __syncthreads();
    for (uint32_t q = 0; q < Z.nreq; q++) {
        uint32_t* L = grp_lds + Z.ldsOff[q]; const uint32_t r = rows[q];
        for (uint32_t i = tid; i < r; i += T) { L[i] = Z.sorted[q][i]; L[Z.limit[q] + i] = 0u; }
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
            uint32_t* L = grp_lds + Z.ldsOff[q];
#pragma unroll
            for (int j = 0; j < LST_GROUP; j++) {
                if (!sw_member(m, j)) continue;
                const uint32_t pos = gh_find(L, r, gc[j]);
                if (pos != GH_NONE) atomicAdd(L + Z.limit[q] + pos, 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t q = 0; q < Z.nreq; q++) {
        const uint32_t* L = grp_lds + Z.ldsOff[q]; const uint32_t r = rows[q];
        for (uint32_t i = tid; i < r; i += T) { const uint32_t x = L[Z.limit[q] + i]; if (x) atomicAdd(Z.sizes[q] + Z.perm[q][i], x); }
    }
}
