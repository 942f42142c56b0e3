// field_quantiles: the sort rank at position floor((count - 1) * q) of a numeric column over the documents a filter accepts, for up to 16 quantiles of the
// whole set and of every value of a second column (infx_field_quantiles).  Included by infidex_hip.hip after groups.hip.inc.  Not in the reference: the
// quantiles are this project's.
//
// The set is a byte per document, 0 = in the set, as in stats.hip.inc.  A member's key is 1 + its sort rank; a rank below nanRanks is a NaN, counted and in
// no quantile.  A SLOT is one group code of a request, and behind the groups (or alone, without a group column) the whole set; a TARGET is one (slot,
// quantile).  All targets of all requests of a call are selected together, most significant digit first, by the arithmetic of quantile_select.h:
//   k_quant_hist   ONE launch per pass for all requests that still have a pass to go (at most QNT_MAX_REQS).  A thread takes 16 consecutive documents
//                  (set_walk.h); inside the walk the requests run one after another: one that shares its predecessor's mask keeps the flag bytes, one that
//                  shares mask and value column keeps the ranks — the host orders a call's requests by (mask, value column, group column).
//                  Pass 0 counts a member's first digit in the ONE row of its slot (every target is under the empty prefix) or in the row's NaN counter;
//                  a later pass counts its digit in the row of every target of its slot whose prefix equals the member's higher digits, as k_list_hist
//                  does for its two targets.  The host places rows in LDS while they fit, exactly as k_field_stats' slots (sts_place: 16 384 words per
//                  workgroup of 256, else the whole LDS of a CU under one workgroup of 1024), else in global memory, hit directly — a request's groups' rows
//                  and the whole set's rows apart: every member of a grouped request meets on the whole set's few bins, which fit where a thousand groups' do
//                  not.  LDS rows are merged at the end with one global atomic per bin that is not zero.
//   k_quant_pick   between the passes, on the stream: one wave per slot.  After pass 0 the row's sum is the slot's count, which turns every q into its
//                  position (qs_position: one double multiplication and its truncation, the only floating-point operation of the call); every pass extends
//                  each target's prefix by the digit that holds its position and keeps the residue.  A request's last pass writes the answers' ranks.
// Integer atomics add to bins; no position is decided by one.
#include "quantile_select.h"
#include "set_walk.h"
#define QNT_MAX_REQS 16
#define QNT_PICK_THREADS 256                // four waves: four slots per workgroup
#define QNT_SCRATCH_WORDS (1u << 24)        // 64 MiB: what the rows of one pass of a call may take in global memory; the digit width is lowered until they fit
struct DevQuantReq {
    const uint8_t* mask;                    // one byte per document, 0 = in the set
    const uint32_t* codes; const uint32_t* rank;      // the value column and its sort rank
    const uint32_t* gcodes;                 // the group column; nullptr: one slot
    const double* q;                        // nq quantiles
    ls_target* tgt;                         // slots x nq targets
    uint32_t* tab;                          // this pass's rows in global memory (zeroed): slots x qs_slot_words
    uint32_t* slotOut;                      // slots x {count, nan}
    uint32_t* rankOut;                      // slots x nq answered ranks
    uint32_t nvals, gvals, slots, nq;       // gvals: values of the group column (0 without one); slots = gvals + 1: the whole set is the last
    uint32_t digitBits, passes, nanRanks;
    uint32_t ldsOff, ldsOffWhole, reuse, slot0;      // the first word in the workgroup's LDS of the groups' rows / of the whole set's, or STS_GLOBAL (placed apart: the whole set's
                                            // few rows take every member of the request and fit where 1000 groups' do not); reuse as DevStatsReq's; slot0: slots of the requests before
};
struct DevQuantCall { uint32_t nreq, slots; DevQuantReq r[QNT_MAX_REQS]; };      // slots: of all requests

// One count for the member of key k (not 0) in a slot of request R in a pass after the first — rows: the slot's nq rows, tg: its nq targets: in the row of every
// target under whose prefix it lies
__device__ __forceinline__ void qnt_count(const DevQuantReq& R, uint32_t* rows, const ls_target* tg, uint32_t k, uint32_t shift) {
    const uint32_t w = R.digitBits, dg = ls_digit(k, shift, w);
    for (uint32_t t = 0; t < R.nq; t++)
        if (ls_under_prefix(k, tg[t].prefix, shift, w)) atomicAdd(rows + ((size_t)t << w) + dg, 1u);      // (a dead target's prefix matches no key)
}
// the words of request R's groups' rows and of the whole set's in a pass
__device__ __forceinline__ uint32_t qnt_slot_words(const DevQuantReq& R, uint32_t pass) { return qs_slot_words(pass, R.nq, R.digitBits); }

// every tab of P zeroed.  Dynamic LDS: the rows of the requests placed there.
__global__ __launch_bounds__(STS_BIG_THREADS) void k_quant_hist(DevQuantCall P, int32_t n, uint32_t pass) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qnt_lds[];
    const int tid = threadIdx.x; const uint32_t T = blockDim.x;      // STS_THREADS, or STS_BIG_THREADS
    for (uint32_t q = 0; q < P.nreq; q++) {
        const DevQuantReq& R = P.r[q];
        const uint32_t sw = qnt_slot_words(R, pass);
        if (R.ldsOff != STS_GLOBAL) for (uint32_t i = tid; i < R.gvals * sw; i += T) qnt_lds[R.ldsOff + i] = 0u;
        if (R.ldsOffWhole != STS_GLOBAL) for (uint32_t i = tid; i < sw; i += T) qnt_lds[R.ldsOffWhole + i] = 0u;
    }
    __syncthreads();
    const int64_t groups = ((int64_t)n + SW_GROUP - 1) / SW_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * T + tid; g < groups; g += (int64_t)gridDim.x * T) {
        const int64_t d0 = g * SW_GROUP;
        uint32_t m[4] = {0, 0, 0, 0}, rr[SW_GROUP];
        bool any = false;
        for (uint32_t q = 0; q < P.nreq; q++) {
            const DevQuantReq& R = P.r[q];
            if (!(R.reuse & 1u)) sw_flags16(R.mask, n, d0, m);
            if (!(R.reuse & 2u)) {
                uint32_t cc[SW_GROUP];
                any = sw_codes16(R.codes, n, d0, m, cc);
#pragma unroll
                for (int j = 0; j < SW_GROUP; j++) rr[j] = any && sw_member(m, j) && cc[j] < R.nvals ? R.rank[cc[j]] : RB_NO_RANK;
            }
            if (!any) continue;
            const uint32_t w = R.digitBits, shift = ls_shift(pass, R.passes, w), sw = qnt_slot_words(R, pass);
            uint32_t* const tabG = R.ldsOff != STS_GLOBAL ? qnt_lds + R.ldsOff : R.tab;                                        // the groups' rows, by group code
            uint32_t* const tabW = R.ldsOffWhole != STS_GLOBAL ? qnt_lds + R.ldsOffWhole : R.tab + (size_t)R.gvals * sw;      // the whole set's
            const ls_target* const tgW = R.tgt + (size_t)R.gvals * R.nq;
            uint32_t gc[SW_GROUP];
            if (R.gcodes) sw_codes16(R.gcodes, n, d0, m, gc);
#pragma unroll
            for (int j = 0; j < SW_GROUP; j++) {
                if (rr[j] == RB_NO_RANK) continue;
                const uint32_t k = qs_key(rr[j], R.nanRanks);
                const bool grouped = R.gcodes && gc[j] < R.gvals;
                if (pass == 0) {
                    const uint32_t bin = k ? ls_digit(k, shift, w) : sw - 1u;        // (the NaN counter lies behind the bins)
                    atomicAdd(tabW + bin, 1u);
                    if (grouped) atomicAdd(tabG + (size_t)gc[j] * sw + bin, 1u);
                } else if (k) {
                    qnt_count(R, tabW, tgW, k, shift);
                    if (grouped) qnt_count(R, tabG + (size_t)gc[j] * sw, R.tgt + (size_t)gc[j] * R.nq, k, shift);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t q = 0; q < P.nreq; q++) {
        const DevQuantReq& R = P.r[q];
        const uint32_t sw = qnt_slot_words(R, pass), gw = R.gvals * sw;
        if (R.ldsOff != STS_GLOBAL) for (uint32_t i = tid; i < gw; i += T) { const uint32_t x = qnt_lds[R.ldsOff + i]; if (x) atomicAdd(R.tab + i, x); }
        if (R.ldsOffWhole != STS_GLOBAL) for (uint32_t i = tid; i < sw; i += T) { const uint32_t x = qnt_lds[R.ldsOffWhole + i]; if (x) atomicAdd(R.tab + gw + i, x); }
    }
}

// the wave's inclusive sum of one value per lane; *total the sum of all
__device__ __forceinline__ uint32_t qnt_wave_scan(uint32_t v, int lane, uint32_t* total) {
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { const uint32_t x = __shfl_up(incl, off); incl += lane >= off ? x : 0u; }
    *total = __shfl(incl, WAVE - 1);
    return incl;
}
// One wave per slot of the call (P.slots in all), every lane a part of the row: (nb + 63) / 64 consecutive bins.  tab: the rows k_quant_hist filled in this pass.
__global__ __launch_bounds__(QNT_PICK_THREADS) void k_quant_pick(DevQuantCall P, uint32_t pass) {
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t s = blockIdx.x * (QNT_PICK_THREADS / WAVE) + (threadIdx.x / WAVE);      // (uniform over the wave)
    if (s >= P.slots) return;
    uint32_t q = 0;
    while (q + 1 < P.nreq && s >= P.r[q + 1].slot0) q++;
    const DevQuantReq& R = P.r[q];
    const uint32_t slot = s - R.slot0, w = R.digitBits, nb = 1u << w, per = (nb + WAVE - 1) / WAVE;
    const uint32_t b0 = min((uint32_t)lane * per, nb), b1 = min(b0 + per, nb);
    const bool last = pass + 1 == R.passes;
    uint32_t count = 0, sum = 0, excl = 0;
    for (uint32_t t = 0; t < R.nq; t++) {
        const uint32_t* row = R.tab + (pass ? ((size_t)slot * R.nq + t) << w : (size_t)slot * qs_row0(w));
        if (pass || !t) {                                                   // pass 0: one row for all targets of the slot, summed once
            uint32_t total;
            sum = 0;
            for (uint32_t b = b0; b < b1; b++) sum += row[b];
            excl = qnt_wave_scan(sum, lane, &total) - sum;
            if (!pass) {
                count = total;
                if (lane == 0) { R.slotOut[2 * (size_t)slot] = count; R.slotOut[2 * (size_t)slot + 1] = row[nb]; }
            }
        }
        const ls_target cur = pass ? R.tgt[(size_t)slot * R.nq + t] : qs_start(count, R.q[t]);
        ls_target next;
        const bool mine = qs_step(cur, row + b0, b0, b1 - b0, excl, w, &next);
        const bool none = !__ballot(mine);                                  // a slot without a non-NaN member: dead from pass 0 on
        if (none) { next.prefix = QS_DEAD; next.resid = 0u; }
        if (mine || (none && lane == 0)) {
            R.tgt[(size_t)slot * R.nq + t] = next;
            if (last) R.rankOut[(size_t)slot * R.nq + t] = qs_rank(next);
        }
    }
}
