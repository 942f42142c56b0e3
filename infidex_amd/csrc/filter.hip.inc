// Infiscript post-filter + facet aggregation on device-resident columns (include/infidex_hip.h, "config 5").  Included by infidex_hip.hip.
//   k_filter_count_multi  FilterVM.Execute of K programs over ALL documents of a range (Filter.NumberOfDocumentsInFilter, ResultProcessor.cs:39-54)
//                         in one launch: each document's codes of the columns any program reads are loaded once into the thread's LDS slots, the K
//                         programs run one after another with wave-uniform control flow, ballot + popcount per wave into per-workgroup LDS counters,
//                         one global atomic per (workgroup, program).  infx_filter_count is the case K = 1.
//   k_filter_mask_multi   the same evaluation written out per document: mask[k][g] = Deleted(g) || !accept_k(g), the per-query Deleted flags of a pre-filter
//                         (Query.pre_filter: "rank only the documents the filter accepts"), four documents per thread, + the count of live accepted documents
//   k_postfilter          ResultProcessor.ApplyFilter on the <= k rows a search returns (:56-69) + FacetBuilder.BuildFacetForField (:58-105): one wave
//                         per query, one row per lane; ballot compaction keeps the row order; facet values are counted with wave shuffles.  Each
//                         query reads its own descriptor (DevQPost: filter program or none, facets on or off); the session-wide setters stage one
//                         descriptor that every query shares.
//   k_postfilter_wide     the same for a query flagged QP_WIDE (an index configured with infx_set_post_rows, a query asking for more than
//                         INFX_FILTER_MAX_ROWS rows): one workgroup per query, up to INFX_POST_MAX_ROWS rows held in registers, row order kept by a
//                         per-wave ballot + a prefix over the wave totals in LDS; facet values counted by an all-pairs pass over the kept rows' codes
//                         in LDS.  k_postfilter skips those queries, k_postfilter_wide every other one.
struct DevFilter {
    const infx_filter_op* ops; uint32_t nops;
    const infx_filter_leaf* leaves; uint32_t nleaves;
    const uint32_t* tables;
};
struct DevColumns { const uint32_t* codes[FILT_MAXCOL]; };

// three-valued evaluation (F = 0, T = 1, N = 2 "not a bool") of the postfix program for one document; code(col) = the document's code in column col.
// The stack is 2 bits per entry in one 64-bit word, top in the low bits (infx_filter_create bounds the depth at 32): a byte array indexed by the
// stack pointer cost the boost loop of k_postproc its SGPR budget.
template <class Code> __device__ __forceinline__ bool filt_eval_codes(const DevFilter& f, Code code) {
    uint64_t st = 0; int sp = 0;
    for (uint32_t i = 0; i < f.nops; i++) {
        const infx_filter_op o = f.ops[i];
        switch (o.op) {
            case INFX_FOP_LEAF: {
                const infx_filter_leaf L = f.leaves[o.arg];
                const uint32_t c = L.col == 0xFFFFFFFFu ? 0u : code(L.col);
                const uint32_t bit = c < L.num_values ? (f.tables[L.table_off + (c >> 5)] >> (c & 31)) & 1u : 0u;
                if (sp < 32) { st = (st << 2) | bit; sp++; }
                break; }
            case INFX_FOP_LIT: if (sp < 32) { st = (st << 2) | 2u; sp++; } break;
            case INFX_FOP_NOT: if (sp >= 1) st = (st & ~3ull) | ((st & 3u) == 1 ? 0u : 1u); break;
            case INFX_FOP_AND: if (sp >= 2) { const uint32_t r = (uint32_t)st & 3u, l = (uint32_t)(st >> 2) & 3u; st >>= 2; sp--; st = (st & ~3ull) | (l == 0 ? 0u : r); } break;
            case INFX_FOP_OR: if (sp >= 2) { const uint32_t r = (uint32_t)st & 3u, l = (uint32_t)(st >> 2) & 3u; st >>= 2; sp--; st = (st & ~3ull) | (l == 1 ? 1u : r); } break;
            case INFX_FOP_TERN: if (sp >= 3) { const uint32_t b = (uint32_t)st & 3u, a = (uint32_t)(st >> 2) & 3u, c = (uint32_t)(st >> 4) & 3u; st >>= 4; sp -= 2; st = (st & ~3ull) | (c == 0 ? b : a); } break;
        }
    }
    return sp > 0 && (st & 3u) == 1;
}
// ... of one document (global internal id), its codes read from the columns
__device__ __forceinline__ bool filt_eval(const DevFilter& f, const DevColumns& cols, int32_t doc) {
    return filt_eval_codes(f, [&](uint32_t c) { return cols.codes[c][doc]; });
}

// The columns the K programs of one k_filter_count_multi launch read: col[u] for u < nUsed, slot[c] = u for column c = col[u]
struct DevCountCols { uint32_t nUsed; uint32_t col[FILT_MAXCOL]; uint8_t slot[FILT_MAXCOL]; };
#define FCM_THREADS 256
// counts[k] += documents of [docBase, docBase + n) that are not Deleted and that program progs[k] accepts, k < K.  Dynamic LDS: K + nUsed * 256 words.
__global__ __launch_bounds__(FCM_THREADS) void k_filter_count_multi(const DevFilter* __restrict__ progs, uint32_t K, DevCountCols cc, DevColumns cols,
                                                                     int32_t docBase, int32_t n, const uint8_t* __restrict__ deleted, uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t fcm_lds[];
    uint32_t* cnt = fcm_lds;                      // per-workgroup count of each program
    uint32_t* codes = fcm_lds + K;                // [u * FCM_THREADS + thread]: the codes of the thread's current document (read back by the same thread only)
    const int tid = threadIdx.x;
    for (uint32_t k = tid; k < K; k += FCM_THREADS) cnt[k] = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * FCM_THREADS; base < n; base += (int64_t)gridDim.x * FCM_THREADS) {
        const int64_t d = base + tid;
        const int32_t g = docBase + (int32_t)(d < n ? d : 0);
        // GetAllDocuments() is the documents that are not Deleted (Core/DocumentCollection.cs:216-219): flagged documents are not counted
        const bool live = d < n && !(deleted && deleted[g]);
        for (uint32_t u = 0; u < cc.nUsed; u++) codes[u * FCM_THREADS + tid] = live ? cols.codes[cc.col[u]][g] : 0u;
        for (uint32_t k = 0; k < K; k++) {
            const DevFilter f = progs[k];
            const bool hit = filt_eval_codes(f, [&](uint32_t c) { return codes[(uint32_t)cc.slot[c] * FCM_THREADS + tid]; }) && live;
            const unsigned long long b = __ballot(hit);
            if ((tid & (WAVE - 1)) == 0 && b) atomicAdd(&cnt[k], (uint32_t)__popcll(b));
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < K; k += FCM_THREADS) if (cnt[k]) atomicAdd(&counts[k], cnt[k]);
}

// ---- pre-filter masks: "for this query, every document the filter rejects is Deleted" (infx_filter_masks) ----
// mask[k][g] = Deleted(g) || !accept_k(g) for every document g of the corpus and K <= INFX_MAX_PREFILTERS programs in ONE pass: a thread takes four consecutive
// documents, so the codes of a column arrive as one 16-byte load and each program's four results leave as one dword store (the masks are padded to a multiple
// of four bytes; the padding reads as rejected).  The last, partial group of a corpus reads its codes and flags one by one: the columns and the Deleted flags
// are not padded.  counts[k] += live accepted documents: ballot + popcount per wave, an LDS counter per workgroup, one global atomic per (workgroup, program).
// Dynamic LDS: (nUsed * 4 * blockDim.x + K) words — the thread's codes, one word per (column, document), laid out lane-fastest; read back by the same thread only.  The host launches 256
// threads while that stays within 40 KiB (four workgroups per CU), else one wave per workgroup (64 columns: 64 KiB).
#define FMM_THREADS 256
struct DevMaskOut { uint8_t* mask[INFX_MAX_PREFILTERS]; };
// The four-document walk of k_filter_mask_multi and k_facets_filtered: thread tid of T takes group gi = documents [d0, d0 + 4) of n
struct FiltGroup4 {
    int64_t d0; bool have, full;       // the group exists; all four of its documents do
    uint32_t dead;                     // byte j: document d0 + j is Deleted, or lies beyond the corpus
    // four consecutive codes of a column: one 16-byte load in a full group, one by one in the corpus's partial last group (columns are not padded)
    __device__ __forceinline__ uint4 load4(const uint32_t* __restrict__ col, int64_t n) const {
        uint4 c = make_uint4(0, 0, 0, 0);
        if (full) c = *(const uint4*)(col + d0);
        else if (have) { c.x = col[d0]; if (d0 + 1 < n) c.y = col[d0 + 1]; if (d0 + 2 < n) c.z = col[d0 + 2]; }      // (d0 + 3 >= n in a partial group)
        return c;
    }
};
// forms the group and leaves the codes of the columns the programs read in codes[(u * 4 + j) * T + tid]: document j, column slot u — consecutive lanes, consecutive banks
__device__ __forceinline__ FiltGroup4 filt_group4(int64_t gi, int64_t groups, int64_t n, const uint8_t* __restrict__ deleted, const DevCountCols& cc, const DevColumns& cols,
                                                  uint32_t* codes, int tid, int T) {
    FiltGroup4 g; g.d0 = gi * 4; g.have = gi < groups; g.full = g.have && g.d0 + 4 <= n; g.dead = 0;
    if (!g.have) g.dead = 0x01010101u;
    else if (g.full) { if (deleted) g.dead = *(const uint32_t*)(deleted + g.d0); }
    else for (int j = 0; j < 4; j++) if (g.d0 + j >= n || (deleted && deleted[g.d0 + j])) g.dead |= 1u << (8 * j);
    for (uint32_t u = 0; u < cc.nUsed; u++) {
        const uint4 c = g.load4(cols.codes[cc.col[u]], n);
        uint32_t* cu = codes + (size_t)u * 4u * T + tid;
        cu[0] = c.x; cu[T] = c.y; cu[2 * T] = c.z; cu[3 * T] = c.w;
    }
    return g;
}
__global__ __launch_bounds__(FMM_THREADS) void k_filter_mask_multi(const DevFilter* __restrict__ progs, uint32_t K, DevCountCols cc, DevColumns cols, int32_t n,
                                                                    const uint8_t* __restrict__ deleted, DevMaskOut out, uint32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fmm_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    uint32_t* codes = fmm_lds;                               // the thread's codes (filt_group4)
    uint32_t* cnt = fmm_lds + (size_t)cc.nUsed * 4u * T;     // per-workgroup count of each program
    for (uint32_t k = tid; k < K; k += T) cnt[k] = 0;
    __syncthreads();
    const int64_t groups = ((int64_t)n + 3) >> 2;
    for (int64_t gb = (int64_t)blockIdx.x * T; gb < groups; gb += (int64_t)gridDim.x * T) {
        const FiltGroup4 g = filt_group4(gb + tid, groups, n, deleted, cc, cols, codes, tid, T);
        for (uint32_t k = 0; k < K; k++) {
            const DevFilter f = progs[k];
            uint32_t word = 0, hits = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool acc = filt_eval_codes(f, [&](uint32_t c) { return codes[((uint32_t)cc.slot[c] * 4u + j) * T + tid]; });
                const bool hit = acc && !((g.dead >> (8 * j)) & 0xFFu);
                hits += (uint32_t)__popcll(__ballot(hit));
                word |= (hit ? 0u : 1u) << (8 * j);
            }
            if (g.have) *(uint32_t*)(out.mask[k] + g.d0) = word;
            if ((tid & (WAVE - 1)) == 0 && hits) atomicAdd(&cnt[k], hits);
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < K; k += T) if (cnt[k]) atomicAdd(&counts[k], cnt[k]);
}

// ---- per-query post-processing (k_postfilter, k_postproc) ----
#define QP_FACETS INFX_QP_FACETS           // count the facet columns of the kept rows
#define QP_SORT   INFX_QP_SORT             // Query.SortBy set (sortCol 0xFFFFFFFF: no such field)
#define QP_ASC    INFX_QP_ASC              // Query.SortAscending
#define QP_WIDE   8u                       // internal: post-processing on more than INFX_FILTER_MAX_ROWS rows (the finalize sets it; the *_wide kernels take the query)
#define QP_REJECTED INFX_RESULT_REJECTED   // result flag of a query whose post-processing needs more rows than the index is configured for
struct DevQPost { int32_t filter; uint32_t flags; uint32_t sortCol; uint32_t boostOff; uint32_t nboost; uint32_t pad[3]; };   // filter: program index, -1 none
struct DevQBoost { int32_t prog; int32_t strength; };
// One batch's post-processing, staged on the stream by the finalize that launches the kernels
struct DevPostBatch {
    const DevFilter* progs; const DevQBoost* boosts; const DevQPost* desc; uint32_t descStride;       // query q: desc[q * descStride] (0: shared by all)
    const uint32_t* rank[FILT_MAXCOL];                                                                // sort ranks of the columns (nullptr: not uploaded)
    // rows of query q: [q * stride, + counts[q]), counts[q] <= INFX_FILTER_MAX_ROWS (QP_WIDE: the index's post rows) for a query with post-processing — filtered, boosted, reordered in place
    long long* keys; float* scores; uint8_t* ties; int32_t* docs; uint32_t* counts; uint32_t* flags; int32_t stride;
    // the batch's fused queries when it has browse queries (INFX_FQ_BROWSE: their rows take no boosts and no sort-by, SearchEngine.cs:292-293), else nullptr
    const infx_fused_query* fqs;
};

// facets of query q, column c: fCodes / fCounts [(q * nfacet + c) * frows ..] (frows: the index's post rows), fN[q * nfacet + c] (0 for a query without facets)
__global__ __launch_bounds__(WAVE) void k_postfilter(const DevPostBatch* __restrict__ pb, DevColumns cols, int nfacet, const uint32_t* __restrict__ facetCols,
                                                      uint32_t* __restrict__ fCodes, uint32_t* __restrict__ fCounts, uint32_t* __restrict__ fN, uint32_t frows) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const DevQPost D = pb->desc[(size_t)q * pb->descStride];
    const bool haveFilter = D.filter >= 0, facets = (D.flags & QP_FACETS) != 0 && nfacet > 0;
    if (!facets && lane < nfacet) fN[(size_t)q * nfacet + lane] = 0;           // (also for a QP_WIDE query: k_postfilter_wide is not launched for a batch whose wide queries only have boosts / sort-by)
    if (D.flags & QP_WIDE) return;                                              // k_postfilter_wide's
    if (!haveFilter && !facets) return;                                         // no post-filter: the rows pass through, whatever their number
    uint32_t* counts = pb->counts;
    if (counts[q] > (uint32_t)WAVE) {                                           // more rows than one wave holds: the query is rejected (empty, flag bit 4)
        if (lane == 0) { counts[q] = 0; pb->flags[q] |= QP_REJECTED; }
        if (facets && lane < nfacet) fN[(size_t)q * nfacet + lane] = 0;
        return;
    }
    const uint32_t n = counts[q];
    const size_t o = (size_t)q * pb->stride;
    long long* keys = pb->keys; float* scores = pb->scores; uint8_t* ties = pb->ties; int32_t* docs = pb->docs;
    const bool have = (uint32_t)lane < n;
    long long k = 0; float s = 0.f; uint8_t t = 0; int32_t d = 0;
    if (have) { k = keys[o + lane]; s = scores[o + lane]; if (ties) t = ties[o + lane]; d = docs[o + lane]; }
    bool keep = have;
    if (haveFilter) { const DevFilter f = pb->progs[D.filter]; keep = have && filt_eval(f, cols, d); }
    const unsigned long long bal = __ballot(keep);
    const uint32_t pos = (uint32_t)__popcll(bal & ((1ull << lane) - 1));
    if (keep) { keys[o + pos] = k; scores[o + pos] = s; if (ties) ties[o + pos] = t; docs[o + pos] = d; }      // every read above happened before any write
    if (lane == 0) counts[q] = (uint32_t)__popcll(bal);
    if (!facets) return;
    for (int c = 0; c < nfacet; c++) {
        const uint32_t code = keep ? cols.codes[facetCols[c]][d] : 0xFFFFFFFFu;
        uint32_t cnt = 0; bool first = keep;
        for (int j = 0; j < WAVE; j++) {
            const uint32_t cj = (uint32_t)__shfl((int)code, j);
            if (keep && cj == code) { cnt++; if (j < lane) first = false; }
        }
        const unsigned long long fb = __ballot(first);
        const size_t fo = ((size_t)q * nfacet + c) * frows;
        if (first) { const uint32_t p = (uint32_t)__popcll(fb & ((1ull << lane) - 1)); fCodes[fo + p] = code; fCounts[fo + p] = cnt; }
        if (lane == 0) fN[(size_t)q * nfacet + c] = (uint32_t)__popcll(fb);
    }
}

// ---- the same on up to INFX_POST_MAX_ROWS rows: one workgroup per query ----
#define PW_THREADS 256
#define PW_ROWS (INFX_POST_MAX_ROWS / PW_THREADS)      // rows per thread: row j * PW_THREADS + thread, j < PW_ROWS
// Ordered compaction over the workgroup: item (j, thread) precedes (j', thread') iff j < j' or j == j' and thread < thread' — the row order.
// pos[j] = set flags before item (j, thread); returns their total.  wtot: PW_ROWS * (PW_THREADS / WAVE) words of LDS, free again on return.
__device__ __forceinline__ uint32_t pw_compact(const bool (&f)[PW_ROWS], uint32_t (&pos)[PW_ROWS], uint32_t* wtot) {
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) {
        const unsigned long long b = __ballot(f[j]);
        pos[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1));
        if (lane == 0) wtot[j * (PW_THREADS / WAVE) + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t run = 0;
    _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++)
        _Pragma("unroll") for (int w = 0; w < PW_THREADS / WAVE; w++) { if (w == wave) pos[j] += run; run += wtot[j * (PW_THREADS / WAVE) + w]; }
    __syncthreads();
    return run;
}
// cap: the index's post rows (<= INFX_POST_MAX_ROWS), also the stride of the facet pairs
__global__ __launch_bounds__(PW_THREADS) void k_postfilter_wide(const DevPostBatch* __restrict__ pb, DevColumns cols, int nfacet, const uint32_t* __restrict__ facetCols,
                                                                 uint32_t* __restrict__ fCodes, uint32_t* __restrict__ fCounts, uint32_t* __restrict__ fN, uint32_t cap) {
    __shared__ uint32_t wtot[PW_ROWS * (PW_THREADS / WAVE)];
    __shared__ uint32_t fcode[INFX_POST_MAX_ROWS];                              // the kept rows' codes of one facet column, in row order
    const int q = blockIdx.x, tid = threadIdx.x;
    const DevQPost D = pb->desc[(size_t)q * pb->descStride];
    if (!(D.flags & QP_WIDE)) return;                                           // k_postfilter's
    const bool haveFilter = D.filter >= 0, facets = (D.flags & QP_FACETS) != 0 && nfacet > 0;
    if (!facets && tid < nfacet) fN[(size_t)q * nfacet + tid] = 0;
    if (!haveFilter && !facets) return;
    uint32_t* counts = pb->counts;
    const uint32_t n = counts[q];
    if (n > cap || n > (uint32_t)INFX_POST_MAX_ROWS) {                          // more rows than the index is configured for: rejected (empty, flag bit 4)
        if (tid == 0) { counts[q] = 0; pb->flags[q] |= QP_REJECTED; }
        if (facets && tid < nfacet) fN[(size_t)q * nfacet + tid] = 0;
        return;
    }
    const size_t o = (size_t)q * pb->stride;
    long long* keys = pb->keys; float* scores = pb->scores; uint8_t* ties = pb->ties; int32_t* docs = pb->docs;
    long long k[PW_ROWS]; float s[PW_ROWS]; uint8_t t[PW_ROWS]; int32_t d[PW_ROWS]; bool keep[PW_ROWS]; uint32_t pos[PW_ROWS];
    DevFilter f{}; if (haveFilter) f = pb->progs[D.filter];
    _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) {
        const uint32_t r = (uint32_t)(j * PW_THREADS + tid);
        const bool have = r < n;
        k[j] = 0; s[j] = 0.f; t[j] = 0; d[j] = 0;
        if (have) { k[j] = keys[o + r]; s[j] = scores[o + r]; if (ties) t[j] = ties[o + r]; d[j] = docs[o + r]; }
        keep[j] = have && (!haveFilter || filt_eval(f, cols, d[j]));
    }
    const uint32_t kept = pw_compact(keep, pos, wtot);                          // its barriers: every row of the query is in registers before any is written
    _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) if (keep[j]) { const size_t w = o + pos[j]; keys[w] = k[j]; scores[w] = s[j]; if (ties) ties[w] = t[j]; docs[w] = d[j]; }
    if (tid == 0) counts[q] = kept;
    if (!facets) return;
    for (int c = 0; c < nfacet; c++) {
        const uint32_t* __restrict__ col = cols.codes[facetCols[c]];
        uint32_t code[PW_ROWS];
        _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) { code[j] = 0xFFFFFFFFu; if (keep[j]) { code[j] = col[d[j]]; fcode[pos[j]] = code[j]; } }
        __syncthreads();
        // kept row i = pos[j]: how many kept rows carry its code, and whether an earlier one does (n^2 / 256 compares per thread)
        uint32_t cnt[PW_ROWS]; bool first[PW_ROWS]; uint32_t fpos[PW_ROWS];
        _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) {
            cnt[j] = 0; first[j] = keep[j];
            if (keep[j]) for (uint32_t m = 0; m < kept; m++) if (fcode[m] == code[j]) { cnt[j]++; if (m < pos[j]) first[j] = false; }
        }
        const uint32_t nd = pw_compact(first, fpos, wtot);                      // (its barriers also free fcode for the next column)
        const size_t fo = ((size_t)q * nfacet + c) * cap;
        _Pragma("unroll") for (int j = 0; j < PW_ROWS; j++) if (first[j]) { fCodes[fo + fpos[j]] = code[j]; fCounts[fo + fpos[j]] = cnt[j]; }
        if (tid == 0) fN[(size_t)q * nfacet + c] = nd;
    }
}
