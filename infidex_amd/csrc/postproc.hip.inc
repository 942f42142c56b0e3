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
//   k_postproc_wide  the same for a query flagged QP_WIDE (up to INFX_POST_MAX_ROWS rows): one workgroup per query.  All threads compute the boosted
//     scores and the sort keys into LDS; then ONE lane runs the same introsort sequence (bcl_introsort_wide) over the permutation in LDS — the sort is
//     unstable, so the sequence of compares and swaps is the result and no parallel sort may stand in for it; then all threads gather the rows through
//     the permutation and, after a barrier, write them back.  k_postproc skips those queries, k_postproc_wide every other one.
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
    if (flags & QP_WIDE) return;                                                // k_postproc_wide's
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

// the sequence accessor of bclsort.hip.inc over LDS (one lane runs the sort); MODE as PpLanes
template <int MODE> struct PpLds {
    int* perm; const int* v; int* frames;      // perm[i]: the row at position i; v[r]: row r's score (float bits, MODE 0) or sort key; frames: BCL_WIDE_MAX_FRAMES slots
    __device__ __forceinline__ int get(int i) const { return perm[i]; }
    __device__ __forceinline__ void set(int i, int x) { perm[i] = x; }
    __device__ __forceinline__ int fget(int i) const { return frames[i]; }
    __device__ __forceinline__ void fset(int i, int x) { frames[i] = x; }
    __device__ __forceinline__ int cmp(int a, int b) const {
        if (MODE == 0) return bcl_cmp_float(__int_as_float(v[b]), __int_as_float(v[a]));
        const uint32_t x = (uint32_t)v[a], y = (uint32_t)v[b];
        return MODE == 1 ? bcl_cmp_u32(x, y) : bcl_cmp_u32(y, x);
    }
};
template <int MODE> __device__ __forceinline__ void pp_sort_lds(int* perm, const int* v, int* frames, int n) {
    PpLds<MODE> L{perm, v, frames};
    bcl_introsort_wide(L, n);
}
// cap: the index's post rows (<= INFX_POST_MAX_ROWS).  Static LDS: 3 x 4 KiB + the frames.
__global__ __launch_bounds__(PW_THREADS) void k_postproc_wide(const DevPostBatch* __restrict__ pb, DevColumns cols, uint32_t cap) {
    __shared__ int sc[INFX_POST_MAX_ROWS], sk[INFX_POST_MAX_ROWS], perm[INFX_POST_MAX_ROWS], frames[BCL_WIDE_MAX_FRAMES];
    const int q = blockIdx.x, tid = threadIdx.x;
    const DevQPost* __restrict__ D = pb->desc + (size_t)q * pb->descStride;
    const uint32_t nboost = D->nboost, flags = D->flags;
    if (!(flags & QP_WIDE)) return;                                             // k_postproc's
    if (!nboost && !(flags & QP_SORT)) return;
    if (pb->fqs && (pb->fqs[q].flags & INFX_FQ_BROWSE)) return;                 // browse rows take no boosts and no sort-by
    const uint32_t cnt = pb->counts[q];
    if (cnt > cap || cnt > (uint32_t)INFX_POST_MAX_ROWS) {                      // more rows than the index is configured for: rejected (empty, flag bit 4)
        if (tid == 0) { pb->counts[q] = 0; pb->flags[q] |= QP_REJECTED; }
        return;
    }
    const int n = (int)cnt;
    const size_t o = (size_t)q * pb->stride;
    long long* keys = pb->keys; float* scores = pb->scores; uint8_t* ties = pb->ties; int32_t* docs = pb->docs;
    const uint32_t col = D->sortCol;
    const uint32_t* rank = (flags & QP_SORT) && col < FILT_MAXCOL ? pb->rank[col] : nullptr;     // nullptr: no such field, every row null
    const DevQBoost* __restrict__ bl = pb->boosts + D->boostOff;
    for (int r = tid; r < n; r += PW_THREADS) {
        float s = scores[o + r]; const int32_t d = docs[o + r];
        uint32_t key = 0;
        if (rank) key = 1u + rank[cols.codes[col][d]];                          // the sort value of the row's document, before the boosts move it
        if (nboost) {
            uint32_t total = 0;                                                 // int arithmetic of the reference (wraps like unchecked C#)
            for (uint32_t b = 0; b < nboost; b++) { const DevQBoost B = bl[b]; if (filt_eval(pb->progs[B.prog], cols, d)) total += (uint32_t)B.strength; }
            if ((int32_t)total > 0) s = s + (float)(int32_t)total;             // float newScore = result.Score + totalBoost
        }
        sc[r] = __float_as_int(s); sk[r] = (int)key; perm[r] = r;
    }
    __syncthreads();
    if (tid == 0) {                                                             // the BCL's sequence, serially
        if (nboost) pp_sort_lds<0>(perm, sc, frames, n);
        if (flags & QP_SORT) { if (flags & QP_ASC) pp_sort_lds<1>(perm, sk, frames, n); else pp_sort_lds<2>(perm, sk, frames, n); }
    }
    __syncthreads();
    long long k2[PW_ROWS]; int32_t d2[PW_ROWS]; uint8_t t2[PW_ROWS]; int s2[PW_ROWS];
    _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) {
        const int i = j * PW_THREADS + tid;
        k2[j] = 0; d2[j] = 0; t2[j] = 0; s2[j] = 0;
        if (i < n) { const int p = perm[i]; k2[j] = keys[o + p]; d2[j] = docs[o + p]; if (ties) t2[j] = ties[o + p]; s2[j] = sc[p]; }
    }
    __syncthreads();                                                            // every row is read before any is written in place
    _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) {
        const int i = j * PW_THREADS + tid;
        if (i < n) { keys[o + i] = k2[j]; scores[o + i] = __int_as_float(s2[j]); if (ties) ties[o + i] = t2[j]; docs[o + i] = d2[j]; }
    }
}
