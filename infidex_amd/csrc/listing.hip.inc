// list_documents: positions [offset, offset + limit) of the documents a filter accepts, in the order (sort key of a column, document), without sorting them
// (infx_list_ordered).  Included by infidex_hip.hip after facets_filtered.hip.inc.  Not in the reference: the order and the paging are this project's.
//
// The set is a byte per document, 0 = in the set: a pre-filter mask (k_filter_mask_multi) or the index's Deleted flags (nullptr: every document).  The key
// of a document is 1 + rank[code] of the ordered column (mirrored for descending; constant without a column), the order (key, document): total, so a page
// is a set of documents and every step below may find it in any order.  The arithmetic is listing_select.h's, shared with the host model.
//   k_list_hist    one pass of a radix select from the most significant digit, for the page's first and last position at once: per-workgroup LDS histograms
//                  (2 x 2^digit_bits words) of the current digit over the documents under each target's prefix, merged with one global atomic per bin
//                  that is not zero.  A thread takes 16 consecutive documents (set_walk.h).
//   k_list_pick    one workgroup, between the passes, on the stream: scans each target's bins, extends its prefix by the digit that holds its position and
//                  keeps the position inside that bin.  The first pass's histogram also gives the size of the set, hence the last position.  After the
//                  last pass: the thresholds T_lo / T_hi and the tie indices (ls_page).
//   k_list_count   browse's structure: workgroup r owns a contiguous run of whole 1024-document tiles and counts its documents of the three classes
//                  (k == T_lo, T_lo < k < T_hi, k == T_hi).
//   k_list_prefix  per class the exclusive prefix over the ranges, and the class totals.
//   k_list_gather  one wave per range that holds a wanted document (every range with a document strictly between the thresholds, whatever the filter: for a wide
//                  page over a many-valued column that is one more pass over the set's ranges, one wave per workgroup): 16 documents per lane, a wave prefix of the lanes' class counts, each wanted document
//                  (key << 32 | document) at the slot ls_slot derives from its index inside its class.  Exactly `count` slots are written, each once.
//   k_list_sort    one workgroup: bitonic sort of the page's <= 1024 composites in LDS (the order is total: any correct sort gives these rows), then
//                  DocumentKey, document and the column's code per row.
// Integer atomics add to histogram bins and range counters; no position is decided by one.
#include "listing_select.h"
#include "set_walk.h"
#define LST_THREADS 256
#define LST_GROUP SW_GROUP                  // documents per thread and step
#define LST_TILE (WAVE * LST_GROUP)         // a wave's step; ranges are runs of whole tiles
#define LST_MAXRANGES 2048u
struct DevListReq {
    const uint8_t* mask;                    // one byte per document, 0 = in the set; nullptr: every document
    const uint32_t* codes; const uint32_t* rank;      // the ordered column and its sort rank; nullptr: constant key (document order)
    uint32_t nvals, ascending, offset, limit, digitBits, passes;
};
struct DevListState { ls_target t[2]; uint32_t total, last, live, pad; ls_page page; uint32_t classTotal[3]; };      // zeroed before the first pass

// keys of the 16 documents from d0 (a multiple of 16) into kk, 0 = not in the set; false: no member among them.  The walk is set_walk.h's.
__device__ __forceinline__ bool lst_keys16(const DevListReq& R, int32_t n, int64_t d0, uint32_t (&kk)[LST_GROUP]) {
    uint32_t m[4], cc[LST_GROUP];
    sw_flags16(R.mask, n, d0, m);
    const bool any = sw_codes16(R.codes, n, d0, m, cc);
#pragma unroll
    for (int j = 0; j < LST_GROUP; j++) kk[j] = sw_member(m, j) ? ls_key(R.rank, cc[j], R.nvals, R.ascending != 0) : 0u;
    return any;
}
__device__ __forceinline__ int32_t lst_range_start(uint32_t r, uint32_t tiles, uint32_t nRanges, int32_t n) {
    return (int32_t)min((int64_t)((uint64_t)r * tiles / nRanges) * LST_TILE, (int64_t)n);
}

// hist: this pass's [2][2^digitBits] global bins (zeroed).  Dynamic LDS: the same.
__global__ __launch_bounds__(LST_THREADS) void k_list_hist(DevListReq R, int32_t n, uint32_t pass, const DevListState* __restrict__ st, uint32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lst_lds[];
    const int tid = threadIdx.x;
    const uint32_t nb = 1u << R.digitBits;
    if (pass && !st->live) return;                                          // an empty page (offset >= total): decided by the first pick
    for (uint32_t i = tid; i < 2u * nb; i += LST_THREADS) lst_lds[i] = 0;
    __syncthreads();
    const ls_target lo = st->t[0], hi = st->t[1];
    const uint32_t shift = ls_shift(pass, R.passes, R.digitBits);
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * LST_THREADS + tid; g < groups; g += (int64_t)gridDim.x * LST_THREADS) {
        uint32_t kk[LST_GROUP];
        if (!lst_keys16(R, n, g * LST_GROUP, kk)) continue;
#pragma unroll
        for (int j = 0; j < LST_GROUP; j++) {
            const uint32_t k = kk[j];
            if (!k) continue;
            const uint32_t dg = ls_digit(k, shift, R.digitBits);
            if (ls_under_prefix(k, lo.prefix, shift, R.digitBits)) atomicAdd(&lst_lds[dg], 1u);
            if (ls_under_prefix(k, hi.prefix, shift, R.digitBits)) atomicAdd(&lst_lds[nb + dg], 1u);      // counted per target also while the prefixes coincide
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 2u * nb; i += LST_THREADS) { const uint32_t x = lst_lds[i]; if (x) atomicAdd(&hist[i], x); }
}

// inclusive scan of one value per thread over the workgroup (part: LST_THREADS words); returns the thread's inclusive sum, *total the sum of all
__device__ __forceinline__ uint32_t lst_block_scan(uint32_t v, uint32_t* part, uint32_t* total) {
    const int tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    for (int off = 1; off < LST_THREADS; off <<= 1) {
        const uint32_t x = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    const uint32_t incl = part[tid]; *total = part[LST_THREADS - 1];
    __syncthreads();
    return incl;
}
__global__ __launch_bounds__(LST_THREADS) void k_list_pick(DevListReq R, uint32_t pass, DevListState* __restrict__ st, const uint32_t* __restrict__ hist) {
    __shared__ uint32_t part[LST_THREADS];
    __shared__ ls_target res[2];
    const int tid = threadIdx.x;
    const uint32_t nb = 1u << R.digitBits, per = (nb + LST_THREADS - 1) / LST_THREADS;
    if (pass && !st->live) return;
    const ls_target cur[2] = {st->t[0], st->t[1]};
    uint32_t last = pass ? st->last : 0u;
    const uint32_t b0 = min((uint32_t)tid * per, nb), b1 = min(b0 + per, nb);
    for (int t = 0; t < 2; t++) {
        const uint32_t* h = hist + (size_t)t * nb;
        uint32_t s = 0;
        for (uint32_t b = b0; b < b1; b++) s += h[b];
        uint32_t total;
        const uint32_t excl = lst_block_scan(s, part, &total) - s;
        if (pass == 0 && t == 0) {                                          // every member is under the empty prefix: the histogram's sum is the set's size
            const bool live = R.offset < total;
            last = live ? (uint32_t)min((uint64_t)R.offset + R.limit, (uint64_t)total) - 1u : 0u;
            if (tid == 0) { st->total = total; st->last = last; st->live = live ? 1u : 0u; }
            if (!live) return;                                              // (uniform)
        }
        const uint32_t resid = pass ? cur[t].resid : (t == 0 ? R.offset : last);
        if (s && resid >= excl && resid - excl < s) {                       // exactly one thread: resid < the entries under the prefix
            uint32_t dg = 0, rest = 0;
            ls_pick(h + b0, b1 - b0, resid - excl, &dg, &rest);
            res[t].prefix = ls_extend(cur[t].prefix, b0 + dg, R.digitBits); res[t].resid = rest;
        }
    }
    __syncthreads();
    if (tid == 0) {
        st->t[0] = res[0]; st->t[1] = res[1];
        if (pass + 1 == R.passes) st->page = ls_make_page(res[0], res[1], R.offset, last);
    }
}

// rangeCnt[c * nRanges + r]: documents of class c + 1 in range r
__global__ __launch_bounds__(LST_THREADS) void k_list_count(DevListReq R, int32_t n, uint32_t tiles, uint32_t nRanges, const DevListState* __restrict__ st,
                                                             uint32_t* __restrict__ rangeCnt) {
    __shared__ uint32_t cnt[3];
    const int tid = threadIdx.x;
    if (!st->live) return;
    const ls_page P = st->page;
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();
    const int32_t lo = lst_range_start(blockIdx.x, tiles, nRanges, n), hi = lst_range_start(blockIdx.x + 1, tiles, nRanges, n);
    uint32_t c1 = 0, c2 = 0, c3 = 0;
    for (int64_t d0 = (int64_t)lo + (int64_t)tid * LST_GROUP; d0 < hi; d0 += (int64_t)LST_THREADS * LST_GROUP) {
        uint32_t kk[LST_GROUP];
        if (!lst_keys16(R, n, d0, kk)) continue;
#pragma unroll
        for (int j = 0; j < LST_GROUP; j++) { const uint32_t c = ls_class(P, kk[j]); c1 += c == 1u; c2 += c == 2u; c3 += c == 3u; }
    }
    if (c1) atomicAdd(&cnt[0], c1);
    if (c2) atomicAdd(&cnt[1], c2);
    if (c3) atomicAdd(&cnt[2], c3);
    __syncthreads();
    if (tid < 3) rangeCnt[(size_t)tid * nRanges + blockIdx.x] = cnt[tid];
}

// grid 3: class blockIdx.x's exclusive prefix over the ranges and its total
__global__ __launch_bounds__(LST_THREADS) void k_list_prefix(uint32_t nRanges, DevListState* __restrict__ st, const uint32_t* __restrict__ rangeCnt, uint32_t* __restrict__ rangePre) {
    __shared__ uint32_t part[LST_THREADS];
    const uint32_t c = blockIdx.x; const int tid = threadIdx.x;
    if (!st->live) return;
    const uint32_t per = (nRanges + LST_THREADS - 1) / LST_THREADS;
    const uint32_t r0 = min((uint32_t)tid * per, nRanges), r1 = min(r0 + per, nRanges);
    const uint32_t* cn = rangeCnt + (size_t)c * nRanges; uint32_t* p = rangePre + (size_t)c * nRanges;
    uint32_t s = 0;
    for (uint32_t r = r0; r < r1; r++) s += cn[r];
    uint32_t total;
    uint32_t run = lst_block_scan(s, part, &total) - s;
    for (uint32_t r = r0; r < r1; r++) { p[r] = run; run += cn[r]; }
    if (tid == 0) st->classTotal[c] = total;
}

// exclusive prefix of v over the wave's lanes; *total: the wave's sum
__device__ __forceinline__ uint32_t lst_wave_scan(uint32_t v, uint32_t* total) {
    const int lane = threadIdx.x & (WAVE - 1);
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, off); if (lane >= off) x += y; }
    *total = (uint32_t)__shfl((int)x, WAVE - 1);
    return x - v;
}
// grid nRanges, one wave: pairs[slot] = key << 32 | document for the wanted documents of the range
__global__ __launch_bounds__(WAVE) void k_list_gather(DevListReq R, int32_t n, uint32_t tiles, uint32_t nRanges, const DevListState* __restrict__ st,
                                                       const uint32_t* __restrict__ rangeCnt, const uint32_t* __restrict__ rangePre, unsigned long long* __restrict__ pairs) {
    const uint32_t r = blockIdx.x; const int lane = threadIdx.x;
    if (!st->live) return;
    const ls_page P = st->page; const uint32_t eqLo = st->classTotal[0];
    uint32_t base1 = rangePre[r], base2 = rangePre[(size_t)nRanges + r], base3 = rangePre[2 * (size_t)nRanges + r];
    const uint32_t n1 = rangeCnt[r], n2 = rangeCnt[(size_t)nRanges + r], n3 = rangeCnt[2 * (size_t)nRanges + r];
    // a class has wanted documents here if its run of indices [base, base + n) meets the wanted interval
    const bool want1 = n1 && base1 + n1 > P.tieLo && (P.tLo != P.tHi || base1 <= P.tieHi);
    const bool want3 = n3 && base3 <= P.tieHi;
    if (!want1 && !n2 && !want3) return;
    const int32_t lo = lst_range_start(r, tiles, nRanges, n), hi = lst_range_start(r + 1, tiles, nRanges, n);
    for (int64_t tb = lo; tb < hi; tb += LST_TILE) {
        const int64_t d0 = tb + (int64_t)lane * LST_GROUP;
        uint32_t kk[LST_GROUP];
#pragma unroll
        for (int j = 0; j < LST_GROUP; j++) kk[j] = 0;
        if (d0 < hi) lst_keys16(R, n, d0, kk);
        uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
        for (int j = 0; j < LST_GROUP; j++) { const uint32_t c = ls_class(P, kk[j]); c1 += c == 1u; c2 += c == 2u; c3 += c == 3u; }
        uint32_t t1, t2, t3;
        uint32_t i1 = base1 + lst_wave_scan(c1, &t1), i2 = base2 + lst_wave_scan(c2, &t2), i3 = base3 + lst_wave_scan(c3, &t3);
        if (c1 | c2 | c3) {
#pragma unroll
            for (int j = 0; j < LST_GROUP; j++) {
                const uint32_t c = ls_class(P, kk[j]);
                if (!c) continue;
                uint32_t idx;
                if (c == 1u) idx = i1++; else if (c == 2u) idx = i2++; else idx = i3++;
                const uint32_t slot = ls_slot(P, c, idx, eqLo);
                if (slot < P.count && slot < (uint32_t)INFX_POST_MAX_ROWS) pairs[slot] = ((unsigned long long)kk[j] << 32) | (uint32_t)(d0 + j);
            }
        }
        base1 += t1; base2 += t2; base3 += t3;
    }
}

// one workgroup: the page's rows in order
#define LST_SORT_THREADS 1024
__global__ __launch_bounds__(LST_SORT_THREADS) void k_list_sort(DevListReq R, int32_t n, const DevListState* __restrict__ st, const unsigned long long* __restrict__ pairs,
                                                                 const long long* __restrict__ docKeyAll, long long* __restrict__ keys, int32_t* __restrict__ docs,
                                                                 uint32_t* __restrict__ codes, uint32_t* __restrict__ count, uint32_t* __restrict__ total) {
    __shared__ unsigned long long v[INFX_POST_MAX_ROWS];
    const uint32_t i = threadIdx.x;
    const uint32_t nrow = st->live ? min(st->page.count, (uint32_t)INFX_POST_MAX_ROWS) : 0u;
    if (i == 0) { *count = nrow; *total = st->total; }
    if (i >= nrow && i < R.limit) { keys[i] = -1; docs[i] = -1; codes[i] = 0u; }      // the rows a caller's buffers hold beyond the page: defined, no document
    if (!nrow) return;
    uint32_t m = 2; while (m < nrow) m <<= 1;                               // the sorted length: a power of two, padded with the largest composite
    v[i] = i < nrow ? pairs[i] : ~0ull;
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
    if (i < nrow) {
        const uint32_t d = (uint32_t)v[i];
        const bool ok = d < (uint32_t)n;                                    // (a slot the gather left untouched reads as all ones: never indexed with)
        keys[i] = ok ? docKeyAll[d] : -1; docs[i] = ok ? (int32_t)d : -1; codes[i] = ok && R.codes ? R.codes[d] : 0u;
    }
}
