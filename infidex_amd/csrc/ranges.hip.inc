// range_facets: bucket counts, below / above / NaN counts and the smallest and largest sort rank of a numeric column over the documents a filter accepts
// (infx_range_counts).  Included by infidex_hip.hip after listing.hip.inc.  Not in the reference: the buckets are this project's.
//
// The set is a byte per document, 0 = in the set: a pre-filter mask (k_filter_mask_multi) or the index's Deleted flags (nullptr: every document).  The work is
// on sort ranks, never on values: the host turns a request's edges into thresholds over the column's dense sort rank (range_buckets.h) and a document of
// rank r = rank[code] goes to the counter rb_slot names.  The arithmetic is range_buckets.h's, shared with the host model.
//   k_range_counts   ONE launch for all requests of a call (at most RB_MAX_REQS).  A thread takes 16 consecutive documents (set_walk.h).
//                    Inside the walk the requests run one after another (the loop and every reuse decision are uniform over the grid): a request that shares
//                    its predecessor's mask keeps the group's flag bytes, one that shares mask and column keeps the ranks too — the host orders a call's
//                    requests by (mask, column).  Per workgroup the thresholds and B + 3 counters of every request lie in LDS with the smallest and largest
//                    non-NaN rank seen; the lookup is rb_upper_bound over the LDS thresholds.  The counters are merged with one global atomic per counter
//                    that is not zero, the ranks with one atomicMin and one atomicMax per request and workgroup.
// Integer atomics add to counters and take a minimum and a maximum; no position is decided by one: any grid and any stream give the same bytes.
#include "range_buckets.h"
#include "set_walk.h"
#define RNG_THREADS 256
#define RNG_OUT_STRIDE 260                  // words per request in the global counters (RB_MAX_SLOTS rounded up to four)
#define RNG_MAXGRID 1024                    // four workgroups per CU, what sixteen requests of 256 buckets leave room for in LDS: every workgroup is resident and merges once
struct DevRangeReq {
    const uint8_t* mask;                    // one byte per document, 0 = in the set; nullptr: every document
    const uint32_t* codes; const uint32_t* rank;      // the column and its sort rank
    const uint32_t* thr;                    // nedges thresholds (device)
    uint32_t nvals, nedges, nanRanks, ldsOff;         // ldsOff: the request's first word in the workgroup's LDS: [thr | counters | min | max]
    uint32_t reuse, pad;                    // bit 0: the mask of the request before, bit 1: its mask and column
};
struct DevRangeCall { uint32_t nreq, pad; DevRangeReq r[RB_MAX_REQS]; };

// sort ranks of the 16 documents from d0 into rr (m: their flags, sw_flags16), RB_NO_RANK = not in the set; false: no member among them
__device__ __forceinline__ bool rng_ranks16(const DevRangeReq& R, int32_t n, int64_t d0, const uint32_t (&m)[4], uint32_t (&rr)[LST_GROUP]) {
    uint32_t cc[LST_GROUP];
    const bool any = sw_codes16(R.codes, n, d0, m, cc);
#pragma unroll
    for (int j = 0; j < LST_GROUP; j++) rr[j] = sw_member(m, j) ? (cc[j] < R.nvals ? R.rank[cc[j]] : 0u) : RB_NO_RANK;
    return any;
}

// cnt: [nreq][RNG_OUT_STRIDE] counters and hi: [nreq] largest ranks (zeroed); lo: [nreq] smallest ranks (all ones).  Dynamic LDS: the requests' words.
__global__ __launch_bounds__(RNG_THREADS) void k_range_counts(DevRangeCall P, int32_t n, uint32_t* __restrict__ cnt, uint32_t* __restrict__ hi, uint32_t* __restrict__ lo) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rng_lds[];
    const int tid = threadIdx.x;
    for (uint32_t q = 0; q < P.nreq; q++) {
        const uint32_t ne = P.r[q].nedges, ns = rb_slots(ne);
        uint32_t* L = rng_lds + P.r[q].ldsOff; const uint32_t* thr = P.r[q].thr;
        for (uint32_t i = tid; i < ne; i += RNG_THREADS) L[i] = thr[i];
        for (uint32_t i = tid; i < ns + 2u; i += RNG_THREADS) L[ne + i] = i == ns ? RB_NO_RANK : 0u;
    }
    __syncthreads();
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * RNG_THREADS + tid; g < groups; g += (int64_t)gridDim.x * RNG_THREADS) {
        const int64_t d0 = g * LST_GROUP;
        uint32_t m[4] = {0, 0, 0, 0}, rr[LST_GROUP];
        bool any = false;
        for (uint32_t q = 0; q < P.nreq; q++) {
            const DevRangeReq& R = P.r[q];
            if (!(R.reuse & 1u)) sw_flags16(R.mask, n, d0, m);
            if (!(R.reuse & 2u)) any = rng_ranks16(R, n, d0, m, rr);
            if (!any) continue;
            const uint32_t ne = R.nedges, nanRanks = R.nanRanks;
            uint32_t* L = rng_lds + R.ldsOff;
            uint32_t* C = L + ne;
            uint32_t mn = RB_NO_RANK, mx = 0u;
#pragma unroll
            for (int j = 0; j < LST_GROUP; j++) {
                const uint32_t r = rr[j];
                if (r == RB_NO_RANK) continue;
                atomicAdd(&C[rb_slot(L, ne, nanRanks, r)], 1u);
                if (r >= nanRanks) { mn = min(mn, r); mx = max(mx, r); }
            }
            if (mn != RB_NO_RANK) {         // both only ever move towards the answer: a stale read skips no update that matters
                volatile uint32_t* E = C + rb_slots(ne);
                if (mn < E[0]) atomicMin(&C[rb_slots(ne)], mn);
                if (mx > E[1]) atomicMax(&C[rb_slots(ne) + 1u], mx);
            }
        }
    }
    __syncthreads();
    for (uint32_t q = 0; q < P.nreq; q++) {
        const uint32_t ne = P.r[q].nedges, ns = rb_slots(ne);
        const uint32_t* C = rng_lds + P.r[q].ldsOff + ne;
        for (uint32_t i = tid; i < ns; i += RNG_THREADS) { const uint32_t x = C[i]; if (x) atomicAdd(&cnt[(size_t)q * RNG_OUT_STRIDE + i], x); }
        if (tid == 0 && C[ns] != RB_NO_RANK) { atomicMin(&lo[q], C[ns]); atomicMax(&hi[q], C[ns + 1u]); }
    }
}
