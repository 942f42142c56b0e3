// field_stats: counts, the smallest and largest sort rank and the EXACT sum of a numeric column over the documents a filter accepts, whole or per value of a
// second column (infx_field_stats).  Included by infidex_hip.hip after ranges.hip.inc.  Not in the reference: the aggregate is this project's.
//
// The set is a byte per document, 0 = in the set, as in ranges.hip.inc.  A member's value code gives bits[code], the 8 raw bytes of its value, and rank[code];
// exact_sum.h turns the bytes into a class (finite, NaN, +inf, -inf), a sign and L unsigned 32-bit limbs of |v| / 2^scale by integer shifts.  A SLOT —
// one per value of the group column, one in all without it — is STS_HEAD + 2 L words: four counters by class, the largest and the smallest non-NaN rank,
// L signed 64-bit limb sums.  Every accumulation is an integer atomic (add, min, max): no floating-point instruction, no order, the same bytes on any grid.
//   k_field_stats    ONE launch for all requests of a call (at most STS_MAX_REQS).  A thread takes 16 consecutive documents (set_walk.h).  Inside the walk the requests run one after another (uniform over the grid): one that
//                    shares its predecessor's mask keeps the flag bytes, one that shares mask and value column keeps the decoded values — the host orders
//                    a call's requests by (mask, value column, group column).
//                    The host places a request's slots in LDS while they fit (requests in ascending size, STS_LDS_WORDS per workgroup of STS_THREADS;
//                    when that leaves a request out that STS_BIG_LDS_WORDS would hold, one workgroup of STS_BIG_THREADS per CU with the whole LDS),
//                    else in global memory, hit directly.  LDS slots are merged at the end: one global atomic per counter or limb sum that is not zero, one atomicMin and
//                    one atomicMax per slot that saw a value.
//                    Without a group column every thread would meet on one slot: a thread adds its 16 documents in registers, the wave reduces by
//                    shuffles, and ONE lane updates the slot per wave and step.  With one, every member is a handful of LDS (or global) atomics on the
//                    slot of its group code.
#include "exact_sum.h"
#include "set_walk.h"
#define STS_THREADS 256
#define STS_BIG_THREADS 1024                // with STS_BIG_LDS_WORDS: one workgroup per CU, the same sixteen waves
#define STS_MAX_REQS 16
#define STS_MAX_GROUPS 4096
#define STS_LDS_WORDS 16384u                // per workgroup, k_facets_all's budget
#define STS_BIG_LDS_WORDS 40960u            // the whole LDS of a CU (gfx950: 160 KiB), for a call whose slots do not fit STS_LDS_WORDS
#define STS_HEAD 6u                         // words of a slot in front of its limb sums: finite, NaN, +inf, -inf, largest rank, smallest rank
#define STS_GLOBAL 0xFFFFFFFFu              // ldsOff of a request whose slots are in global memory
struct DevStatsReq {
    const uint8_t* mask;                    // one byte per document, 0 = in the set; nullptr: every document
    const uint32_t* codes; const uint32_t* rank; const uint64_t* bits;      // the value column, its sort rank and its raw values by code
    const uint32_t* gcodes;                 // the group column; nullptr: one slot
    uint32_t* out;                          // gvals slots of sts_stride(nlimbs) words (zeroed); word 5 of a slot is not used here:
    uint32_t* lo;                           // gvals smallest ranks (all ones)
    uint32_t nvals, gvals, nlimbs; int32_t kind, scale;
    uint32_t ldsOff, reuse, pad;            // ldsOff: the first word of the slots in the workgroup's LDS, or STS_GLOBAL; reuse bit 0: the mask of the request before, bit 1: its mask and value column
};
struct DevStatsCall { uint32_t nreq, pad; DevStatsReq r[STS_MAX_REQS]; };
__host__ __device__ __forceinline__ uint32_t sts_stride(uint32_t nlimbs) { return STS_HEAD + 2u * nlimbs; }

// raw values and sort ranks of the 16 documents from d0 (m: their flags, sw_flags16): vr = RB_NO_RANK marks a document outside the set; false: no member among them
__device__ __forceinline__ bool sts_values16(const DevStatsReq& R, int32_t n, int64_t d0, const uint32_t (&m)[4], uint64_t (&vb)[LST_GROUP], uint32_t (&vr)[LST_GROUP]) {
    uint32_t cc[LST_GROUP];
    const bool any = sw_codes16(R.codes, n, d0, m, cc);
#pragma unroll
    for (int j = 0; j < LST_GROUP; j++) {
        const bool in = any && sw_member(m, j) && cc[j] < R.nvals;
        vb[j] = in ? R.bits[cc[j]] : 0ull;
        vr[j] = in ? R.rank[cc[j]] : RB_NO_RANK;
    }
    return any;
}
// one slot takes counters c by class, the extreme ranks (mn = RB_NO_RANK: none) and limb sums s; lo: where the slot's smallest rank lives.  LDS or global
// memory, by the pointers it is inlined with.  Both ranks only ever move towards the answer: a stale read skips no update that matters.
__device__ __forceinline__ void sts_add(uint32_t* slot, uint32_t* lo, const uint32_t (&c)[4], uint32_t mn, uint32_t mx, const long long (&s)[XS_MAX_LIMBS], uint32_t nlimbs) {
#pragma unroll
    for (int k = 0; k < 4; k++) if (c[k]) atomicAdd(slot + k, c[k]);
    if (mn != RB_NO_RANK) {
        if (mn < *(volatile uint32_t*)lo) atomicMin(lo, mn);
        if (mx > *(volatile uint32_t*)(slot + 4)) atomicMax(slot + 4, mx);
    }
#pragma unroll
    for (int i = 0; i < XS_MAX_LIMBS; i++) if ((uint32_t)i < nlimbs && s[i]) atomicAdd((unsigned long long*)(slot + STS_HEAD) + i, (unsigned long long)s[i]);
}

// every out / lo of P zeroed / all ones.  Dynamic LDS: the slots of the requests placed there.
__global__ __launch_bounds__(STS_BIG_THREADS) void k_field_stats(DevStatsCall P, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sts_lds[];
    const int tid = threadIdx.x; const uint32_t T = blockDim.x;      // STS_THREADS, or STS_BIG_THREADS
    for (uint32_t q = 0; q < P.nreq; q++) {
        if (P.r[q].ldsOff == STS_GLOBAL) continue;
        const uint32_t W = sts_stride(P.r[q].nlimbs), words = P.r[q].gvals * W;
        uint32_t* L = sts_lds + P.r[q].ldsOff;
        for (uint32_t i = tid; i < words; i += T) L[i] = i % W == 5u ? RB_NO_RANK : 0u;
    }
    __syncthreads();
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    // every thread of a workgroup takes the same number of steps (the wave reduction below needs all lanes): a thread past the corpus sees no member
    for (int64_t g0 = (int64_t)blockIdx.x * T; g0 < groups; g0 += (int64_t)gridDim.x * T) {
        const int64_t d0 = (g0 + tid) * LST_GROUP;
        uint32_t m[4] = {0, 0, 0, 0}, vr[LST_GROUP]; uint64_t vb[LST_GROUP];
        bool any = false;
        for (uint32_t q = 0; q < P.nreq; q++) {
            const DevStatsReq& R = P.r[q];
            if (!(R.reuse & 1u)) sw_flags16(R.mask, n, d0, m);
            if (!(R.reuse & 2u)) any = sts_values16(R, n, d0, m, vb, vr);
            const uint32_t nl = R.nlimbs, W = sts_stride(nl);
            const bool inLds = R.ldsOff != STS_GLOBAL;
            if (!R.gcodes) {
                if (!__ballot(any)) continue;                                 // (uniform over the wave)
                uint32_t c[4] = {0, 0, 0, 0}, mn = RB_NO_RANK, mx = 0u; long long s[XS_MAX_LIMBS] = {0, 0, 0, 0};
                if (any) {
#pragma unroll
                    for (int j = 0; j < LST_GROUP; j++) {
                        if (vr[j] == RB_NO_RANK) continue;
                        uint32_t neg, limb[XS_MAX_LIMBS];
                        const uint32_t cls = xs_limbs(vb[j], R.kind, R.scale, &neg, limb);
#pragma unroll
                        for (int k = 0; k < 4; k++) c[k] += cls == (uint32_t)k ? 1u : 0u;
                        if (cls != XS_NAN) { mn = min(mn, vr[j]); mx = max(mx, vr[j]); }
#pragma unroll
                        for (int i = 0; i < XS_MAX_LIMBS; i++) s[i] += neg ? -(long long)limb[i] : (long long)limb[i];
                    }
                }
#pragma unroll
                for (int off = WAVE / 2; off; off >>= 1) {
#pragma unroll
                    for (int k = 0; k < 4; k++) c[k] += __shfl_xor(c[k], off);
                    mn = min(mn, __shfl_xor(mn, off)); mx = max(mx, __shfl_xor(mx, off));
#pragma unroll
                    for (int i = 0; i < XS_MAX_LIMBS; i++) if ((uint32_t)i < nl) s[i] += __shfl_xor(s[i], off);
                }
                if ((tid & (WAVE - 1)) == 0) {
                    if (inLds) sts_add(sts_lds + R.ldsOff, sts_lds + R.ldsOff + 5u, c, mn, mx, s, nl);
                    else sts_add(R.out, R.lo, c, mn, mx, s, nl);
                }
                continue;
            }
            if (!any) continue;
            uint32_t gc[LST_GROUP];
            sw_codes16(R.gcodes, n, d0, m, gc);
#pragma unroll
            for (int j = 0; j < LST_GROUP; j++) {
                if (vr[j] == RB_NO_RANK || gc[j] >= R.gvals) continue;
                uint32_t neg, limb[XS_MAX_LIMBS];
                const uint32_t cls = xs_limbs(vb[j], R.kind, R.scale, &neg, limb);
                uint32_t c[4]; long long s[XS_MAX_LIMBS];
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] = cls == (uint32_t)k ? 1u : 0u;
#pragma unroll
                for (int i = 0; i < XS_MAX_LIMBS; i++) s[i] = neg ? -(long long)limb[i] : (long long)limb[i];
                const uint32_t r = cls != XS_NAN ? vr[j] : RB_NO_RANK;
                if (inLds) { uint32_t* S = sts_lds + R.ldsOff + gc[j] * W; sts_add(S, S + 5u, c, r, r, s, nl); }
                else sts_add(R.out + (size_t)gc[j] * W, R.lo + gc[j], c, r, r, s, nl);
            }
        }
    }
    __syncthreads();
    for (uint32_t q = 0; q < P.nreq; q++) {
        const DevStatsReq& R = P.r[q];
        if (R.ldsOff == STS_GLOBAL) continue;
        const uint32_t W = sts_stride(R.nlimbs), words = R.gvals * W;
        const uint32_t* L = sts_lds + R.ldsOff;
        for (uint32_t i = tid; i < words; i += T) {
            const uint32_t k = i % W, x = L[i];
            if (k < 4u) { if (x) atomicAdd(R.out + i, x); }
            else if (k == 4u) { if (x) atomicMax(R.out + i, x); }
            else if (k == 5u) { if (x != RB_NO_RANK) atomicMin(R.lo + i / W, x); }
            else if (!(k & 1u)) { const unsigned long long v = *(const unsigned long long*)(L + i); if (v) atomicAdd((unsigned long long*)(R.out + i), v); }
        }
    }
}
