// List columns: multi-valued document fields in filters and facets (infx_upload_list_column, infx_list_leaf_build, infx_list_facets).
// Included by infidex_hip.hip after facets_filtered.hip.inc.  Reference: Field.IsArray / FacetBuilder.cs:82-91, 143-152 (every element of a list is counted).
//
// A list column is a CSR pair on the device: elemOff[n + 1] (uint32: a column holds fewer than 2^32 elements) and elemCode[total], the dictionary codes of
// the elements in document order, order and duplicates kept.
//
// k_list_leaf lowers up to LL_MAX_LEAVES filter leaves over ONE list column to derived one-bit columns (uint32 bit[n], 0 or 1) in one launch: bit k of a
// document = leaf k holds for at least one element of its list, or, for an empty list, the leaf's verdict on a null value (bit k of emptyBits).  The filter VM
// then reads a derived column as any scalar column of two values: no kernel that runs a program knows about lists.
//   - element-parallel: a workgroup takes LL_DOCS consecutive documents, loads their elemOff window into LDS, and its lanes stride over the window's contiguous
//     element range with coalesced loads of elemCode; a lane finds its element's document by a binary search in the LDS window (8 steps) and ORs the element's
//     K-bit hit word into the document's LDS slot; after a barrier the workgroup writes K coalesced uint32 columns.
//   - the K leaf bitmaps sit side by side, word w of leaf k at maps[w * K + k]: one load of an element's code answers all K leaves from K consecutive words.
//     They are staged in LDS while K * ceil(V / 32) <= INFX_LIST_LEAF_LDS_WORDS (8 KiB), and read from global memory beyond that.
//   - integer ORs only: the result does not depend on the grid or on the order.
// What bounds it: memory traffic — it reads 4 (n + 1) + 4 E bytes and writes 4 K n bytes (E elements, K leaves).  LDS per workgroup: (2 LL_DOCS + 1 +
// INFX_LIST_LEAF_LDS_WORDS) * 4 = 10 244 bytes, 256 threads, so the 8 workgroups (32 waves) a CU can hold stay resident within its 160 KiB.
//
// k_list_facets counts, for up to INFX_MAX_PREFILTERS accept sets, the element occurrences of every value among the accepted documents: counters
// [k][elementCode].  The accept sets are document flags, one byte per document, 1 = rejected or Deleted — the session's pre-filter masks (built by
// infx_filter_masks through the engine's 16-mask cache, which leaves k_facets_filtered untouched), or the Deleted flags for the whole corpus (nullptr: every
// document is accepted).  Same walk as k_list_leaf; a document's K-bit accept word sits in its LDS slot, and an element's code is
// loaded only when its document is in at least one set (a block of documents that is in none is skipped whole).  The counters live in per-workgroup LDS while
// K * V <= FFL_LDS_WORDS (k_facets_filtered's budget; infx_list_facets decides), merged with one global atomic per non-zero counter, and in global memory beyond it.
// Integer adds only: the bytes are the same from any run, session or grid.
#define LL_THREADS 256
#define LL_DOCS 256                      // documents of one workgroup block
#define LL_MAX_LEAVES 16
#define LL_MAXGRID 2048
struct DevListLeaf {
    const uint32_t* elemOff; const uint32_t* elemCode; const uint32_t* maps;      // maps: [ceil(V / 32)][K]
    uint32_t* out[LL_MAX_LEAVES];
    uint32_t K, nvals, emptyBits, mapsInLds; int32_t n;
};
// the document of element e in the block's offset window off[0 .. nd]: the last i with off[i] <= e (off[i + 1] > e follows, empty lists are skipped)
__device__ __forceinline__ uint32_t ll_doc_of(const uint32_t* off, uint32_t nd, uint32_t e) {
    uint32_t lo = 0, hi = nd;            // invariant: off[lo] <= e < off[hi]
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (off[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(LL_THREADS) void k_list_leaf(DevListLeaf A) {
    __shared__ uint32_t off[LL_DOCS + 1];
    __shared__ uint32_t hit[LL_DOCS];
    __shared__ uint32_t mapsLds[INFX_LIST_LEAF_LDS_WORDS];
    const uint32_t tid = threadIdx.x, K = A.K;
    const uint32_t mapWords = ((A.nvals + 31u) >> 5) * K;
    if (A.mapsInLds) for (uint32_t i = tid; i < mapWords; i += LL_THREADS) mapsLds[i] = A.maps[i];
    const uint32_t* maps = A.mapsInLds ? mapsLds : A.maps;
    const int64_t blocks = ((int64_t)A.n + LL_DOCS - 1) / LL_DOCS;
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t d0 = b * LL_DOCS;
        const uint32_t nd = (uint32_t)min((int64_t)LL_DOCS, (int64_t)A.n - d0);
        __syncthreads();                 // the previous block's window is written out (and the bitmaps are staged)
        for (uint32_t i = tid; i <= nd; i += LL_THREADS) off[i] = A.elemOff[d0 + i];
        if (tid < nd) hit[tid] = 0;
        __syncthreads();
        const uint64_t e0 = off[0], e1 = off[nd];
        for (uint64_t e = e0 + tid; e < e1; e += LL_THREADS) {
            const uint32_t c = A.elemCode[e];
            if (c >= A.nvals) continue;
            const uint32_t* w = maps + (size_t)(c >> 5) * K;
            uint32_t word = 0;
            for (uint32_t k = 0; k < K; k++) word |= ((w[k] >> (c & 31u)) & 1u) << k;
            if (word) atomicOr(&hit[ll_doc_of(off, nd, (uint32_t)e)], word);
        }
        __syncthreads();
        if (tid < nd) {
            const uint32_t word = off[tid] == off[tid + 1] ? A.emptyBits : hit[tid];
            for (uint32_t k = 0; k < K; k++) A.out[k][d0 + tid] = (word >> k) & 1u;
        }
    }
}

struct DevListFacets {
    const uint32_t* elemOff; const uint32_t* elemCode;
    const uint8_t* mask[INFX_MAX_PREFILTERS];      // accept set k: 1 = rejected or Deleted; nullptr: every document
    uint32_t* out;                                 // [K][nvals]
    uint32_t K, nvals, inLds; int32_t n;
};
__global__ __launch_bounds__(LL_THREADS) void k_list_facets(DevListFacets A) {
    extern __shared__ uint32_t lf_lds[];
    uint32_t* off = lf_lds;                        // [LL_DOCS + 1]
    uint32_t* acc = off + LL_DOCS + 1;             // [LL_DOCS] accept words
    uint32_t* ctr = acc + LL_DOCS;                 // [K * nvals] when inLds
    const uint32_t tid = threadIdx.x, K = A.K, nv = A.nvals;
    const uint32_t words = A.inLds ? K * nv : 0u;
    for (uint32_t i = tid; i < words; i += LL_THREADS) ctr[i] = 0;
    uint32_t* cnt = A.inLds ? ctr : A.out;
    const int64_t blocks = ((int64_t)A.n + LL_DOCS - 1) / LL_DOCS;
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t d0 = b * LL_DOCS;
        const uint32_t nd = (uint32_t)min((int64_t)LL_DOCS, (int64_t)A.n - d0);
        __syncthreads();
        for (uint32_t i = tid; i <= nd; i += LL_THREADS) off[i] = A.elemOff[d0 + i];
        uint32_t mine = 0;
        if (tid < nd) {
            for (uint32_t k = 0; k < K; k++) { const uint8_t* m = A.mask[k]; mine |= ((m ? m[d0 + tid] : (uint8_t)0) ? 0u : 1u) << k; }
            acc[tid] = mine;
        }
        if (!__syncthreads_or((int)(mine != 0))) continue;      // no set accepts a document of this block: its elements are not read (workgroup-uniform)
        const uint64_t e0 = off[0], e1 = off[nd];
        for (uint64_t e = e0 + tid; e < e1; e += LL_THREADS) {
            uint32_t w = acc[ll_doc_of(off, nd, (uint32_t)e)];
            if (!w) continue;                                    // (nor are the elements of a document that no set accepts)
            const uint32_t c = A.elemCode[e];
            if (c >= nv) continue;
            while (w) {
                const uint32_t k = (uint32_t)__builtin_ctz(w); w &= w - 1;
                atomicAdd(cnt + (size_t)k * nv + c, 1u);
            }
        }
    }
    if (A.inLds) {
        __syncthreads();
        for (uint32_t i = tid; i < words; i += LL_THREADS) { const uint32_t x = ctr[i]; if (x) atomicAdd(A.out + i, x); }
    }
}
