// bucket_stats: field_stats' figures — counts by class, the extreme sort ranks and the EXACT limb sums of a numeric column — per RANGE BUCKET of a second
// numeric column, over the documents a filter accepts (infx_bucket_stats).  Included by infidex_hip.hip after stats.hip.inc.  Not in the reference: the
// aggregate is this project's.
//
// The set is a byte per document, 0 = in the set, as in ranges.hip.inc and stats.hip.inc.  A member's value code gives its raw value and sort rank
// (sts_values16); its bucket column's code gives brank[code], and rb_slot over the request's thresholds names one of the request's B + 3 slots
// [below | B buckets | above | nan] (bucket_stats.h, shared with the host model).  A slot is field_stats' slot and takes the member through sts_add: integer
// atomics only (add, min, max), no floating-point instruction, no atomic that decides a position — the same bytes on any grid and placement.
//   k_bucket_stats   ONE launch for all requests of a call (at most BKS_MAX_REQS).  A thread takes 16 consecutive documents (set_walk.h).  Inside the walk the
//                    requests run one after another (uniform over the grid): one that shares its predecessor's mask keeps the flag bytes, one that shares
//                    mask and value column keeps the decoded values — the host orders a call's requests by (mask, value column, bucket column).
//                    The thresholds of every request lie in LDS, in front; the slots are placed by field_stats' rule (sts_place_best) with both budgets
//                    reduced by the thresholds: in LDS while they fit — 256 threads and STS_LDS_WORDS, or one workgroup of 1024 threads per CU with the
//                    whole LDS — else in global memory, hit directly.  LDS slots are merged at the end as k_field_stats merges them.
//                    With BKS_MERGE_RUNS a thread adds a run of its documents that fall into ONE slot in registers and hits the slot once per run: on a
//                    bucket column that follows the document order every lane of a wave meets on one slot, and sixteen members cost one visit.
#include "bucket_stats.h"
#ifndef BKS_MERGE_RUNS
#define BKS_MERGE_RUNS 1
#endif
static_assert(BKS_HEAD == STS_HEAD && BKS_MAX_REQS == STS_MAX_REQS, "a bucket's slot is field_stats' slot");
struct DevBucketReq {
    DevStatsReq s;                          // the set, the value column and the slots: gcodes the bucket column's codes, gvals the request's B + 3 slots
    const uint32_t* brank;                  // the bucket column's sort rank
    const uint32_t* thr;                    // nedges thresholds (device)
    uint32_t bvals, nedges, nanRanks, thrOff;      // thrOff: the first word of the thresholds in the workgroup's LDS
};
struct DevBucketCall { uint32_t nreq, pad; DevBucketReq r[BKS_MAX_REQS]; };

// every s.out / s.lo of P zeroed / all ones.  Dynamic LDS: the thresholds, then the slots of the requests placed there.
__global__ __launch_bounds__(STS_BIG_THREADS) void k_bucket_stats(DevBucketCall P, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bks_lds[];
    const int tid = threadIdx.x; const uint32_t T = blockDim.x;      // STS_THREADS, or STS_BIG_THREADS
    for (uint32_t q = 0; q < P.nreq; q++) {
        const DevBucketReq& R = P.r[q];
        uint32_t* H = bks_lds + R.thrOff;
        for (uint32_t i = tid; i < R.nedges; i += T) H[i] = R.thr[i];
        if (R.s.ldsOff == STS_GLOBAL) continue;
        const uint32_t W = sts_stride(R.s.nlimbs), words = R.s.gvals * W;
        uint32_t* L = bks_lds + R.s.ldsOff;
        for (uint32_t i = tid; i < words; i += T) L[i] = i % W == 5u ? RB_NO_RANK : 0u;
    }
    __syncthreads();
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * T + tid; g < groups; g += (int64_t)gridDim.x * T) {
        const int64_t d0 = g * LST_GROUP;
        uint32_t m[4] = {0, 0, 0, 0}, vr[LST_GROUP]; uint64_t vb[LST_GROUP];
        bool any = false;
        for (uint32_t q = 0; q < P.nreq; q++) {
            const DevBucketReq& R = P.r[q];
            if (!(R.s.reuse & 1u)) sw_flags16(R.s.mask, n, d0, m);
            if (!(R.s.reuse & 2u)) any = sts_values16(R.s, n, d0, m, vb, vr);
            if (!any) continue;
            const uint32_t nl = R.s.nlimbs, W = sts_stride(nl), ne = R.nedges, nanRanks = R.nanRanks;
            const bool inLds = R.s.ldsOff != STS_GLOBAL;
            const uint32_t* H = bks_lds + R.thrOff;
            uint32_t bc[LST_GROUP];
            sw_codes16(R.s.gcodes, n, d0, m, bc);
            // the slot takes (c, mn, mx, s): in LDS beside its smallest rank, in global memory with that rank in lo
            auto add = [&](uint32_t slot, const uint32_t (&c)[4], uint32_t mn, uint32_t mx, const long long (&s)[XS_MAX_LIMBS]) {
                if (inLds) { uint32_t* S = bks_lds + R.s.ldsOff + slot * W; sts_add(S, S + 5u, c, mn, mx, s, nl); }
                else sts_add(R.s.out + (size_t)slot * W, R.s.lo + slot, c, mn, mx, s, nl);
            };
#if BKS_MERGE_RUNS
            uint32_t cur = RB_NO_RANK, c[4] = {0, 0, 0, 0}, mn = RB_NO_RANK, mx = 0u; long long s[XS_MAX_LIMBS] = {0, 0, 0, 0};
#endif
#pragma unroll
            for (int j = 0; j < LST_GROUP; j++) {
                if (vr[j] == RB_NO_RANK) continue;
                const uint32_t br = bc[j] < R.bvals ? R.brank[bc[j]] : 0u;
                const BksMember M = bks_member(H, ne, nanRanks, br, vb[j], vr[j], R.s.kind, R.s.scale);
#if BKS_MERGE_RUNS
                if (M.slot != cur) {
                    if (cur != RB_NO_RANK) add(cur, c, mn, mx, s);
                    cur = M.slot; mn = RB_NO_RANK; mx = 0u;
#pragma unroll
                    for (int k = 0; k < 4; k++) c[k] = 0u;
#pragma unroll
                    for (int i = 0; i < XS_MAX_LIMBS; i++) s[i] = 0;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] += M.cls == (uint32_t)k ? 1u : 0u;
                if (M.rank != RB_NO_RANK) { mn = min(mn, M.rank); mx = max(mx, M.rank); }
#pragma unroll
                for (int i = 0; i < XS_MAX_LIMBS; i++) s[i] += M.neg ? -(long long)M.limb[i] : (long long)M.limb[i];
#else
                uint32_t c[4]; long long s[XS_MAX_LIMBS];
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] = M.cls == (uint32_t)k ? 1u : 0u;
#pragma unroll
                for (int i = 0; i < XS_MAX_LIMBS; i++) s[i] = M.neg ? -(long long)M.limb[i] : (long long)M.limb[i];
                add(M.slot, c, M.rank, M.rank, s);
#endif
            }
#if BKS_MERGE_RUNS
            if (cur != RB_NO_RANK) add(cur, c, mn, mx, s);
#endif
        }
    }
    __syncthreads();
    for (uint32_t q = 0; q < P.nreq; q++) {
        const DevStatsReq& R = P.r[q].s;
        if (R.ldsOff == STS_GLOBAL) continue;
        const uint32_t W = sts_stride(R.nlimbs), words = R.gvals * W;
        const uint32_t* L = bks_lds + R.ldsOff;
        for (uint32_t i = tid; i < words; i += T) {
            const uint32_t k = i % W, x = L[i];
            if (k < 4u) { if (x) atomicAdd(R.out + i, x); }
            else if (k == 4u) { if (x) atomicMax(R.out + i, x); }
            else if (k == 5u) { if (x != RB_NO_RANK) atomicMin(R.lo + i / W, x); }
            else if (!(k & 1u)) { const unsigned long long v = *(const unsigned long long*)(L + i); if (v) atomicAdd((unsigned long long*)(R.out + i), v); }
        }
    }
}
