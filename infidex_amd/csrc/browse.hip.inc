// Browse rows (SearchEngine.HandleEmptyQueryWithFacets, SearchEngine.cs:321-346) and whole-corpus facets (FacetBuilder.BuildFacetsFromAllDocuments,
// Core/FacetBuilder.cs:110-181) on the device-resident columns.  Included by infidex_hip.hip after filter.hip.inc.
//
// A batch's browse queries (empty text + EnableFacets) are grouped by distinct filter program; group g wants the first rows[g] documents, in internal
// order, that are not Deleted and whose key's first live document the program accepts.  The order comes from the structure of the scan, no atomic
// decides a slot:
//   k_browse_scan    k_filter_count_multi's walk (256 threads, one document per thread per tile, the used columns' codes in LDS slots, the groups'
//                    programs one after another, ballot + popcount), but workgroup r owns the CONTIGUOUS tiles [r * tiles / nRanges, (r + 1) * tiles / nRanges) of 256 documents
//                    and stores its count of every group: rangeCnt[g * nRanges + r].  A group whose Filter.NumberOfDocumentsInFilter the batch
//                    still needs (BRW_COUNT) is evaluated on every document; a group that only needs rows stops inside a range once the range
//                    alone holds rows[g] matches (its stored count is then a lower bound >= rows[g], which is all the prefix needs).
//   k_browse_prefix  per group the exclusive prefix of its range counts; the total is the group's NumberOfDocumentsInFilter.
//   k_browse_gather  one wave per (range, group) whose prefix lies below rows[g] and whose count is not 0: evaluates the range again, 64 documents
//                    per step, ballot compaction -> rowDocs[g * rowStride + prefix + i] (rowStride: the index's post rows).  At most rows[g] ranges
//                    per group do any work.
//   k_browse_rows    one wave per browse query: the first min(total, MaxNumberOfRecordsToReturn) documents of its group become its result rows
//                    (key, score 65535, tiebreaker 0, and the document the post-filter / facets look at) where k_finalize left an empty result.
//   k_browse_rows_wide  the same with one workgroup per query, launched instead when a query of the batch wants more than 64 rows.
// Duplicate keys (firstLive != nullptr): the rows' filter looks at firstLive[d], the first live document carrying d's key
// (ResultProcessor.ApplyFilter -> GetDocumentByPublicKey), while NumberOfDocumentsInFilter evaluates each live document's own fields
// (ResultProcessor.cs:39-54): the DUP instantiation holds both sets of codes and adds the own-field count with one atomic per (range, group).
#define BRW_COUNT 1u            // the group's NumberOfDocumentsInFilter is wanted: no early stop, countsOut[countIdx] is written
#define BRW_THREADS FCM_THREADS
#define BRW_SCORE 65535.0f      // ushort.MaxValue
struct DevBrowseGroup { DevFilter f; int32_t prog; uint32_t rows; uint32_t flags; uint32_t countIdx; };      // prog -1: no filter; f: the program itself (no second table lookup per tile)
struct DevBrowseQuery { uint32_t q; uint32_t group; uint32_t rows; uint32_t pad; };

// first document of range r: the ranges are runs of whole 256-document tiles whose lengths differ by at most one tile (the workgroups finish together)
__device__ __forceinline__ int32_t brw_range_start(uint32_t r, uint32_t tiles, uint32_t nRanges, int32_t n) {
    return (int32_t)min((int64_t)((uint64_t)r * tiles / nRanges) * BRW_THREADS, (int64_t)n);
}
template <bool DUP>
__global__ __launch_bounds__(BRW_THREADS) void k_browse_scan(const DevBrowseGroup* __restrict__ groups, uint32_t G,
                                                              DevCountCols cc, DevColumns cols, int32_t n, uint32_t tiles, uint32_t nRanges,
                                                              const uint8_t* __restrict__ deleted, const int32_t* __restrict__ firstLive, int earlyStop,
                                                              uint32_t* __restrict__ rangeCnt, uint32_t* __restrict__ ownCnt) {
    extern __shared__ uint32_t brw_lds[];
    uint32_t* cnt = brw_lds;                                            // [G] matches of this range (the rows' rule)
    uint32_t* own = brw_lds + G;                                        // [G] DUP only: matches by the documents' own fields
    uint32_t* codes = brw_lds + (DUP ? 2u * G : G);                     // [u * BRW_THREADS + thread]: codes of the document the rows' filter looks at
    uint32_t* ocodes = codes + cc.nUsed * BRW_THREADS;                  // DUP only: codes of the document itself
    const int tid = threadIdx.x;
    for (uint32_t g = tid; g < (DUP ? 2u * G : G); g += BRW_THREADS) brw_lds[g] = 0;
    __syncthreads();
    const int32_t lo = brw_range_start(blockIdx.x, tiles, nRanges, n), hi = brw_range_start(blockIdx.x + 1, tiles, nRanges, n);
    for (int32_t base = lo; base < hi; base += BRW_THREADS) {
        const int32_t d = base + tid < hi ? base + tid : lo;
        const bool live = base + tid < hi && !(deleted && deleted[d]);
        const int32_t rep = DUP && live ? firstLive[d] : d;
        for (uint32_t u = 0; u < cc.nUsed; u++) {
            codes[u * BRW_THREADS + tid] = live ? cols.codes[cc.col[u]][rep] : 0u;
            if (DUP) ocodes[u * BRW_THREADS + tid] = live ? cols.codes[cc.col[u]][d] : 0u;
        }
        bool anyOpen = false;
        for (uint32_t g = 0; g < G; g++) {
            const DevBrowseGroup Gp = groups[g];
            const bool counting = (Gp.flags & BRW_COUNT) != 0;
            // rows only: enough matches in this range already (the value read is a lower bound of the range's count at any moment)
            if (earlyStop && !counting && (uint32_t)__builtin_amdgcn_readfirstlane((int)__atomic_load_n(&cnt[g], __ATOMIC_RELAXED)) >= Gp.rows) continue;
            anyOpen = true;
            bool hit = live;
            if (Gp.prog >= 0) {
                const DevFilter f = Gp.f;
                hit = filt_eval_codes(f, [&](uint32_t c) { return codes[(uint32_t)cc.slot[c] * BRW_THREADS + tid]; }) && live;
                if (DUP && counting) {
                    const bool ohit = filt_eval_codes(f, [&](uint32_t c) { return ocodes[(uint32_t)cc.slot[c] * BRW_THREADS + tid]; }) && live;
                    const unsigned long long ob = __ballot(ohit);
                    if ((tid & (WAVE - 1)) == 0 && ob) atomicAdd(&own[g], (uint32_t)__popcll(ob));
                }
            }
            const unsigned long long b = __ballot(hit);
            if ((tid & (WAVE - 1)) == 0 && b) atomicAdd(&cnt[g], (uint32_t)__popcll(b));
        }
        if (!anyOpen) break;                                            // every group of this launch has its rows (wave-uniform: no barrier inside the loop)
    }
    __syncthreads();
    for (uint32_t g = tid; g < G; g += BRW_THREADS) {
        rangeCnt[(size_t)g * nRanges + blockIdx.x] = cnt[g];
        if (DUP && own[g]) atomicAdd(&ownCnt[g], own[g]);
    }
}

// rangePre[g * nRanges + r] = matches of group g in the ranges before r; totals[g] = all of them (clamped sums cannot overflow: <= documents).
// countsOut[countIdx] = NumberOfDocumentsInFilter of a BRW_COUNT group: the total, or with duplicate keys the own-field count.
__global__ __launch_bounds__(BRW_THREADS) void k_browse_prefix(const DevBrowseGroup* __restrict__ groups, uint32_t nRanges, const uint32_t* __restrict__ rangeCnt,
                                                                const uint32_t* __restrict__ ownCnt, uint32_t* __restrict__ rangePre,
                                                                uint32_t* __restrict__ totals, uint32_t* __restrict__ countsOut) {
    __shared__ uint32_t part[BRW_THREADS];
    const uint32_t g = blockIdx.x; const int tid = threadIdx.x;
    const uint32_t per = (nRanges + BRW_THREADS - 1) / BRW_THREADS;    // consecutive ranges per thread
    const uint32_t r0 = min((uint32_t)tid * per, nRanges), r1 = min(r0 + per, nRanges);
    const uint32_t* c = rangeCnt + (size_t)g * nRanges; uint32_t* p = rangePre + (size_t)g * nRanges;
    uint32_t s = 0;
    for (uint32_t r = r0; r < r1; r++) s += c[r];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < BRW_THREADS; off <<= 1) {                   // inclusive scan of the 256 partial sums
        const uint32_t v = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - s;
    for (uint32_t r = r0; r < r1; r++) { p[r] = run; run += c[r]; }
    if (tid == BRW_THREADS - 1) {
        const DevBrowseGroup Gp = groups[g];
        totals[g] = part[tid];
        if (Gp.flags & BRW_COUNT) countsOut[Gp.countIdx] = ownCnt ? ownCnt[g] : part[tid];
    }
}

// grid (nRanges, Y), one wave: the documents of range blockIdx.x that group g keeps, written at their rank among all of g's documents
__global__ __launch_bounds__(WAVE) void k_browse_gather(const DevBrowseGroup* __restrict__ groups, uint32_t G, DevColumns cols,
                                                         int32_t n, uint32_t tiles, uint32_t nRanges, const uint8_t* __restrict__ deleted,
                                                         const int32_t* __restrict__ firstLive, const uint32_t* __restrict__ rangeCnt,
                                                         const uint32_t* __restrict__ rangePre, int32_t* __restrict__ rowDocs, uint32_t rowStride) {
    const uint32_t r = blockIdx.x; const int lane = threadIdx.x;
    const int32_t lo = brw_range_start(r, tiles, nRanges, n), hi = brw_range_start(r + 1, tiles, nRanges, n);
    for (uint32_t g = blockIdx.y; g < G; g += gridDim.y) {
        const DevBrowseGroup Gp = groups[g];
        uint32_t pos = rangePre[(size_t)g * nRanges + r];
        if (pos >= Gp.rows || rangeCnt[(size_t)g * nRanges + r] == 0) continue;
        const DevFilter f = Gp.f;
        for (int32_t base = lo; base < hi && pos < Gp.rows; base += WAVE) {
            const int32_t d = base + lane < hi ? base + lane : lo;
            const bool live = base + lane < hi && !(deleted && deleted[d]);
            bool hit = live;
            if (Gp.prog >= 0) { const int32_t rep = firstLive && live ? firstLive[d] : d; hit = filt_eval(f, cols, rep) && live; }
            const unsigned long long b = __ballot(hit);
            const uint32_t p = pos + (uint32_t)__popcll(b & ((1ull << lane) - 1));
            if (hit && p < Gp.rows) rowDocs[(size_t)g * rowStride + p] = d;
            pos += (uint32_t)__popcll(b);
        }
    }
}

// one wave per browse query: its rows (at most 64), where k_finalize wrote an empty result (counts 0, flags 0)
__global__ __launch_bounds__(WAVE) void k_browse_rows(const DevBrowseQuery* __restrict__ bq, const DevBrowseGroup* __restrict__ groups, const uint32_t* __restrict__ totals,
                                                       const int32_t* __restrict__ rowDocs, uint32_t rowStride, const long long* __restrict__ docKeyAll, const int32_t* __restrict__ firstLive,
                                                       int32_t stride, long long* __restrict__ keys, float* __restrict__ scores, uint8_t* __restrict__ ties,
                                                       int32_t* __restrict__ docs, uint32_t* __restrict__ counts) {
    const DevBrowseQuery Q = bq[blockIdx.x]; const uint32_t lane = threadIdx.x;
    const uint32_t nrow = min(min(totals[Q.group], groups[Q.group].rows), min(Q.rows, (uint32_t)stride));
    const size_t o = (size_t)Q.q * stride;
    if (lane < nrow) {
        const int32_t d = rowDocs[(size_t)Q.group * rowStride + lane];
        keys[o + lane] = docKeyAll[d]; scores[o + lane] = BRW_SCORE; if (ties) ties[o + lane] = 0;
        docs[o + lane] = firstLive ? firstLive[d] : d;                  // ApplyFilter and BuildFacets look the row up by key: the key's first live document
    }
    if (lane == 0) counts[Q.q] = nrow;
}
// one workgroup per browse query: up to rowStride rows
__global__ __launch_bounds__(BRW_THREADS) void k_browse_rows_wide(const DevBrowseQuery* __restrict__ bq, const DevBrowseGroup* __restrict__ groups, const uint32_t* __restrict__ totals,
                                                                   const int32_t* __restrict__ rowDocs, uint32_t rowStride, const long long* __restrict__ docKeyAll,
                                                                   const int32_t* __restrict__ firstLive, int32_t stride, long long* __restrict__ keys, float* __restrict__ scores,
                                                                   uint8_t* __restrict__ ties, int32_t* __restrict__ docs, uint32_t* __restrict__ counts) {
    const DevBrowseQuery Q = bq[blockIdx.x];
    const uint32_t nrow = min(min(min(totals[Q.group], groups[Q.group].rows), min(Q.rows, (uint32_t)stride)), rowStride);
    const size_t o = (size_t)Q.q * stride;
    for (uint32_t r = threadIdx.x; r < nrow; r += BRW_THREADS) {
        const int32_t d = rowDocs[(size_t)Q.group * rowStride + r];
        keys[o + r] = docKeyAll[d]; scores[o + r] = BRW_SCORE; if (ties) ties[o + r] = 0;
        docs[o + r] = firstLive ? firstLive[d] : d;
    }
    if (threadIdx.x == 0) counts[Q.q] = nrow;
}

// ---- whole-corpus facets -------------------------------------------------------------------------------------------------------------------
// out[c][v] += live documents whose code in facet column c is v, all columns in ONE pass over the documents.  A column of at most FALL_LDS_VALUES
// distinct values is counted in LDS per workgroup and merged with one global atomic per (workgroup, value that occurred); a larger one adds to its
// global counters directly (integer atomics: the sums do not depend on the order).
#define FALL_THREADS 256
#define FALL_LDS_VALUES 4096u
struct DevFacetAll { const uint32_t* codes[INFX_MAX_FACET_COLS]; uint32_t* out[INFX_MAX_FACET_COLS]; uint32_t nvals[INFX_MAX_FACET_COLS]; uint32_t ldsOff[INFX_MAX_FACET_COLS]; };   // ldsOff 0xFFFFFFFF: global counters
__global__ __launch_bounds__(FALL_THREADS) void k_facets_all(DevFacetAll F, int ncol, uint32_t ldsWords, int32_t n, const uint8_t* __restrict__ deleted) {
    extern __shared__ uint32_t fall_lds[];
    const int tid = threadIdx.x;
    for (uint32_t i = tid; i < ldsWords; i += FALL_THREADS) fall_lds[i] = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * FALL_THREADS; base < n; base += (int64_t)gridDim.x * FALL_THREADS) {
        const int64_t d = base + tid;
        if (d >= n || (deleted && deleted[d])) continue;
        for (int c = 0; c < ncol; c++) {
            const uint32_t v = F.codes[c][d];
            if (v >= F.nvals[c]) continue;
            if (F.ldsOff[c] != 0xFFFFFFFFu) atomicAdd(&fall_lds[F.ldsOff[c] + v], 1u); else atomicAdd(&F.out[c][v], 1u);
        }
    }
    __syncthreads();
    for (int c = 0; c < ncol; c++) if (F.ldsOff[c] != 0xFFFFFFFFu)
        for (uint32_t v = tid; v < F.nvals[c]; v += FALL_THREADS) { const uint32_t x = fall_lds[F.ldsOff[c] + v]; if (x) atomicAdd(&F.out[c][v], x); }
}
