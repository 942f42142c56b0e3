// Query.Boosts + Query.SortBy on the rows a search returns (SearchEngine.cs:348-361 after ApplyFilter).  Included by infidex_hip.hip after filter.hip.inc.
//   k_postproc  one wave per query, one lane per row (<= INFX_FILTER_MAX_ROWS), after k_postfilter:
//     1. ResultProcessor.ApplyBoosts (ResultProcessor.cs:75-121): per row the sum of the strengths of the boost programs its document satisfies
//        (filt_eval), Score = Score + totalBoost as an fp32 add where totalBoost > 0; then Array.Sort by score descending — always, once a boost
//        with a filter is installed, so rows with equal scores move even when none was boosted.
//     2. ResultProcessor.ApplySort (:126-141, CompareValues :180-201): key = 1 + rank[code of the row's document] (0 = null: the field does not exist),
//        Array.Sort with CompareValues(a, b) ascending or CompareValues(b, a) descending.
//   Both sorts are the BCL's unstable introsort (bclsort.hip.inc), run serially over the <= 64 rows with wave-uniform control flow: lane i holds the
//   row at position i and the i-th pending range; an element is read with v_readlane at a uniform index and written with a per-lane select, so the
//   compares and branches are scalar and nothing lives in scratch or LDS.  The permuted rows are gathered with shuffles and written back in place.
//   Each query reads its own descriptor (DevQPost in filter.hip.inc: boost list, sort column and direction) from the batch's DevPostBatch; a query
//   without boosts or sort passes through.  The launch's parameters live in device memory (staged on the stream): as kernel arguments the boost
//   programs and row pointers stayed in scalar registers across filt_eval and the sorts and spilled.
__device__ __forceinline__ int pp_readlane(int v, int i) { return __builtin_amdgcn_readlane(v, i); }
// the sequence accessor of bclsort.hip.inc over the lanes of the wave; MODE 0 score descending, 1 key ascending, 2 key descending
template <int MODE> struct PpLanes {
    int lane, perm, frame;          // perm: the row at position `lane`; frame: slot `lane` of the pending-range stack
    int v;                          // this lane's row: its score (float bits, MODE 0) or its sort key
    __device__ __forceinline__ int get(int i) const { return pp_readlane(perm, i); }
    __device__ __forceinline__ void set(int i, int x) { perm = lane == i ? x : perm; }
    __device__ __forceinline__ int fget(int i) const { return pp_readlane(frame, i); }
    __device__ __forceinline__ void fset(int i, int x) { frame = lane == i ? x : frame; }
    __device__ __forceinline__ int cmp(int a, int b) const {
        if (MODE == 0) return bcl_cmp_float(__int_as_float(pp_readlane(v, b)), __int_as_float(pp_readlane(v, a)));
        const uint32_t x = (uint32_t)pp_readlane(v, a), y = (uint32_t)pp_readlane(v, b);
        return MODE == 1 ? bcl_cmp_u32(x, y) : bcl_cmp_u32(y, x);
    }
};
template <int MODE> __device__ __forceinline__ int pp_sort(int perm, int v, int n) {
    PpLanes<MODE> L{(int)threadIdx.x, perm, 0, v};
    bcl_introsort(L, n);
    return L.perm;
}
__global__ __launch_bounds__(WAVE) void k_postproc(const DevPostBatch* __restrict__ pb, DevColumns cols) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const DevQPost* __restrict__ D = pb->desc + (size_t)q * pb->descStride;
    const uint32_t nboost = D->nboost, flags = D->flags;
    if (!nboost && !(flags & QP_SORT)) return;                                  // nothing to do: the rows pass through, whatever their number
    if (pb->fqs && (pb->fqs[q].flags & INFX_FQ_BROWSE)) return;                 // browse rows: HandleEmptyQueryWithFacets returns before ApplyPostProcessing
    if (pb->counts[q] > (uint32_t)WAVE) {                                       // more rows than one wave holds: the query is rejected (empty, flag bit 4)
        if (lane == 0) { pb->counts[q] = 0; pb->flags[q] |= QP_REJECTED; }
        return;
    }
    const int n = (int)pb->counts[q];
    const bool have = lane < n;
    float s = 0.f; int32_t d = 0;
    if (have) { const size_t o = (size_t)q * pb->stride; s = pb->scores[o + lane]; d = pb->docs[o + lane]; }
    uint32_t key = 0;
    if (flags & QP_SORT) {                                                      // the sort value of the row's document, before the boosts move it
        const uint32_t col = D->sortCol;
        const uint32_t* rank = col < FILT_MAXCOL ? pb->rank[col] : nullptr;     // nullptr: no such field, every row null
        if (have && rank) key = 1u + rank[cols.codes[col][d]];
    }
    if (nboost) {
        const DevQBoost* __restrict__ bl = pb->boosts + D->boostOff;
        uint32_t total = 0;                                                     // int arithmetic of the reference (wraps like unchecked C#)
        if (have) for (uint32_t b = 0; b < nboost; b++) { const DevQBoost B = bl[b]; if (filt_eval(pb->progs[B.prog], cols, d)) total += (uint32_t)B.strength; }
        if ((int32_t)total > 0) s = s + (float)(int32_t)total;                 // float newScore = result.Score + totalBoost
    }
    int perm = lane;                                                            // the row at position `lane`: a permutation of [0, n) on the first n lanes
    if (nboost) perm = pp_sort<0>(perm, __float_as_int(s), n);
    if (flags & QP_SORT) perm = (flags & QP_ASC) ? pp_sort<1>(perm, (int)key, n) : pp_sort<2>(perm, (int)key, n);
    long long* keys = pb->keys; float* scores = pb->scores; uint8_t* ties = pb->ties; int32_t* docs = pb->docs;
    const size_t o = (size_t)q * pb->stride;
    long long k = 0; int t = 0;
    if (have) { k = keys[o + lane]; if (ties) t = ties[o + lane]; }
    const long long k2 = __shfl(k, perm); const float s2 = __shfl(s, perm); const int t2 = __shfl(t, perm); const int32_t d2 = __shfl(d, perm);
    if (have) { keys[o + lane] = k2; scores[o + lane] = s2; if (ties) ties[o + lane] = (uint8_t)t2; docs[o + lane] = d2; }
}
