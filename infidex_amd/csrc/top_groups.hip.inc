// top_groups: the groups of a column over the documents a filter accepts, ranked by a figure of the group — size, count, min, max, sum or mean of a value
// column — and cut to a page (infx_top_groups).  Included by infidex_hip.hip after groups.hip.inc.  Not in the reference: the ranking is this project's.
//
// A TABLE is (mask, value column or none, group column): one slot per code of the group column.  The requests of a call are taken table by table.
//   accumulate      with a value column k_field_stats itself fills the table (one request, field_stats' slots of STS_HEAD + 2 L words and its placement
//                   rule; no cap on the slots).  Without one k_top_sizes: the same walk (set_walk.h), the slot is the member counter.
//   k_top_keys      one thread per group code and request: the slot becomes a composite (top_select.h) — class, figure of `by`, tie — with the sums and means
//                   of exact_sum.h, the functions the host turns slots into figures with.  Counts the rows (groups with a member) and the set's size.
//   k_top_hist      per pass of the radix select, all requests of the table that still have a pass in one launch (grid y): the digit of every composite
//                   under the prefix of either target, in LDS, merged with one atomic per bin that is not zero
//   k_top_pick      one workgroup per request: before pass 0 the two targets from the row count, then one digit more for each; zeroes the histogram
//   k_top_gather    the codes whose composite lies between the two resolved targets: exactly the page, in no order
//   k_top_page      one workgroup per request: the page's composites in LDS, every row's position by counting the smaller ones (composites are distinct),
//                   the codes in order and their slots
// Integer atomics only, none decides an answer's bytes: the gather's order is undone by the sort.
#include "top_select.h"
#define TOP_THREADS 256
#define TOP_MAX_REQS 16
#define TOP_SLOT_WORDS (STS_HEAD + 2u * XS_MAX_LIMBS)       // a row's slot in the answer: 14 words whatever the column's limbs
#define TOP_OUT_HEAD 4u                                     // words in front of a request's rows: page rows, groups with a member, the set's size, 0
#define TOP_OUT_WORDS (TOP_OUT_HEAD + INFX_POST_MAX_ROWS * (1u + TOP_SLOT_WORDS))
struct DevTopState { ts_target t[2]; uint32_t count, gathered; };
struct DevTopReq {
    const uint32_t* slots; const uint32_t* lo;      // the table: gvals slots of `stride` words (stride 1: member counters, lo null), their smallest ranks
    const uint32_t* tie;                            // the group column's facet tie order by code
    uint32_t* keys;                                 // gvals composites of nw words
    uint32_t* hist;                                 // 2 x LS_MAX_BINS bins (zeroed)
    DevTopState* st;                                // (zeroed)
    uint32_t* out;                                  // TOP_OUT_WORDS (zeroed): head, codes, slots
    uint32_t gvals, stride, nlimbs, by; int32_t kind, scale;
    uint32_t ascending, offset, limit, digitBits, figWords, passes;
};
struct DevTopCall { uint32_t nreq, pad; DevTopReq r[TOP_MAX_REQS]; };

// out: gvals member counters (zeroed).  Dynamic LDS: the counters when inLds.
__global__ __launch_bounds__(STS_BIG_THREADS) void k_top_sizes(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ gcodes, uint32_t gvals, uint32_t* __restrict__ out, uint32_t inLds, int32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t top_lds[];
    const int tid = threadIdx.x; const uint32_t T = blockDim.x;      // STS_THREADS, or STS_BIG_THREADS
    if (inLds) for (uint32_t i = tid; i < gvals; i += T) top_lds[i] = 0u;
    __syncthreads();
    const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
    for (int64_t g = (int64_t)blockIdx.x * T + tid; g < groups; g += (int64_t)gridDim.x * T) {
        const int64_t d0 = g * LST_GROUP;
        uint32_t m[4], gc[LST_GROUP];
        sw_flags16(mask, n, d0, m);
        if (!sw_codes16(gcodes, n, d0, m, gc)) continue;
#pragma unroll
        for (int j = 0; j < LST_GROUP; j++) {
            if (!sw_member(m, j) || gc[j] >= gvals) continue;
            if (inLds) atomicAdd(top_lds + gc[j], 1u); else atomicAdd(out + gc[j], 1u);
        }
    }
    __syncthreads();
    if (inLds) for (uint32_t i = tid; i < gvals; i += T) { const uint32_t x = top_lds[i]; if (x) atomicAdd(out + i, x); }
}

// the slot of code g of R's table as ts_figure takes it
__device__ __forceinline__ void top_slot(const DevTopReq& R, uint32_t g, uint32_t (&c)[4], uint32_t* mx, uint32_t* mn, int64_t (&S)[XS_MAX_LIMBS]) {
#pragma unroll
    for (int i = 0; i < XS_MAX_LIMBS; i++) S[i] = 0;
    if (R.stride == 1u) { c[0] = R.slots[g]; c[1] = c[2] = c[3] = 0u; *mx = 0u; *mn = TS_NO_RANK; return; }
    const uint32_t* w = R.slots + (size_t)g * R.stride;
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = w[k];
    *mx = w[4]; *mn = R.lo[g];
#pragma unroll
    for (int i = 0; i < XS_MAX_LIMBS; i++) if ((uint32_t)i < R.nlimbs) S[i] = (int64_t)(((const unsigned long long*)(w + STS_HEAD))[i]);
}

// grid y: the requests of P (one table).  out[1] += rows, out[2] += members
__global__ __launch_bounds__(TOP_THREADS) void k_top_keys(DevTopCall P) {
    __shared__ uint32_t acc[2];
    const DevTopReq& R = P.r[blockIdx.y];
    if (threadIdx.x < 2) acc[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t nw = ts_key_words(R.figWords);
    uint32_t rows = 0, members = 0;
    for (uint32_t g = blockIdx.x * TOP_THREADS + threadIdx.x; g < R.gvals; g += gridDim.x * TOP_THREADS) {
        uint32_t c[4], mx, mn, fig[TS_MAX_FIG], key[TS_MAX_WORDS]; int64_t S[XS_MAX_LIMBS];
        top_slot(R, g, c, &mx, &mn, S);
        const uint32_t cls = ts_figure(R.by, c, mx, mn, S, R.kind, R.scale, R.nlimbs, fig);
        ts_compose(cls, fig, R.figWords, R.ascending != 0, R.tie[g], key);
        uint32_t* K = R.keys + (size_t)g * nw;
#pragma unroll
        for (uint32_t j = 0; j < TS_MAX_WORDS; j++) if (j < nw) K[j] = key[j];
        if (cls != TS_NONE) { rows++; members += c[0] + c[1] + c[2] + c[3]; }
    }
    if (rows) { atomicAdd(&acc[0], rows); atomicAdd(&acc[1], members); }
    __syncthreads();
    if (threadIdx.x == 0 && acc[0]) { atomicAdd(R.out + 1, acc[0]); atomicAdd(R.out + 2, acc[1]); }
}

// a composite of nw words from global memory into registers
__device__ __forceinline__ void top_load(const uint32_t* __restrict__ K, uint32_t nw, uint32_t (&key)[TS_MAX_WORDS]) {
#pragma unroll
    for (uint32_t j = 0; j < TS_MAX_WORDS; j++) key[j] = j < nw ? K[j] : 0u;
}

// grid y: the requests of P, each with a pass `pass` to go.  Dynamic LDS: 2 << digitBits bins (the widest request's).
__global__ __launch_bounds__(TOP_THREADS) void k_top_hist(DevTopCall P, uint32_t pass) {
    extern __shared__ __attribute__((aligned(16))) uint32_t top_bins[];
    __shared__ ts_target tg[2];
    const DevTopReq& R = P.r[blockIdx.y];
    const uint32_t nw = ts_key_words(R.figWords), keyBits = ts_key_bits(R.figWords);
    const uint32_t start = ts_digit_start(pass, R.digitBits), width = ts_digit_width(pass, R.digitBits, keyBits), nb = 1u << width;
    if (threadIdx.x < 2) tg[threadIdx.x] = R.st->t[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < 2u * nb; i += TOP_THREADS) top_bins[i] = 0u;
    __syncthreads();
    if (tg[0].dead && tg[1].dead) return;                          // (uniform over the workgroup)
    for (uint32_t g = blockIdx.x * TOP_THREADS + threadIdx.x; g < R.gvals; g += gridDim.x * TOP_THREADS) {
        uint32_t key[TS_MAX_WORDS];
        top_load(R.keys + (size_t)g * nw, nw, key);
        const uint32_t dg = ts_digit(key, nw, start, width);
        if (!tg[0].dead && ts_under_prefix(key, tg[0].prefix, start)) atomicAdd(top_bins + dg, 1u);
        if (!tg[1].dead && ts_under_prefix(key, tg[1].prefix, start)) atomicAdd(top_bins + nb + dg, 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2u * nb; i += TOP_THREADS) { const uint32_t x = top_bins[i]; if (x) atomicAdd(R.hist + (i < nb ? i : LS_MAX_BINS + (i - nb)), x); }
}

// grid: the requests of P.  Thread t < 2 advances target t by the digit of `pass`; before pass 0 the targets come from the row count k_top_keys left.
__global__ __launch_bounds__(TOP_THREADS) void k_top_pick(DevTopCall P, uint32_t pass) {
    const DevTopReq& R = P.r[blockIdx.x];
    const uint32_t nw = ts_key_words(R.figWords), keyBits = ts_key_bits(R.figWords);
    const uint32_t start = ts_digit_start(pass, R.digitBits), width = ts_digit_width(pass, R.digitBits, keyBits);
    if (threadIdx.x == 0 && pass == 0) {
        ts_target lo, hi;
        R.st->count = ts_start(R.out[1], R.offset, R.limit, &lo, &hi);
        R.st->t[0] = lo; R.st->t[1] = hi;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        ts_target t = R.st->t[threadIdx.x];
        ts_step(&t, R.hist + threadIdx.x * LS_MAX_BINS, nw, start, width);
        R.st->t[threadIdx.x] = t;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2u * LS_MAX_BINS; i += TOP_THREADS) R.hist[i] = 0u;
}

// grid y: the requests of P.  The page's codes land in out's code rows in no order; st->gathered counts them.
__global__ __launch_bounds__(TOP_THREADS) void k_top_gather(DevTopCall P) {
    __shared__ ts_target tg[2];
    const DevTopReq& R = P.r[blockIdx.y];
    const uint32_t nw = ts_key_words(R.figWords);
    if (threadIdx.x < 2) tg[threadIdx.x] = R.st->t[threadIdx.x];
    __syncthreads();
    if (tg[0].dead || tg[1].dead) return;
    for (uint32_t g = blockIdx.x * TOP_THREADS + threadIdx.x; g < R.gvals; g += gridDim.x * TOP_THREADS) {
        uint32_t key[TS_MAX_WORDS];
        top_load(R.keys + (size_t)g * nw, nw, key);
        if (!ts_on_page(key, nw, tg[0], tg[1])) continue;
        const uint32_t at = atomicAdd(&R.st->gathered, 1u);
        if (at < INFX_POST_MAX_ROWS) R.out[TOP_OUT_HEAD + at] = g;
    }
}

// grid: the requests of P; LST_SORT_THREADS threads, one per row of a page.  out: [rows, ., ., . | codes in order | their slots]
__global__ __launch_bounds__(LST_SORT_THREADS) void k_top_page(DevTopCall P) {
    __shared__ uint32_t pk[INFX_POST_MAX_ROWS * TS_MAX_WORDS];
    const DevTopReq& R = P.r[blockIdx.x];
    const uint32_t nw = ts_key_words(R.figWords), i = threadIdx.x;
    const uint32_t nrow = min(min(R.st->gathered, R.st->count), (uint32_t)INFX_POST_MAX_ROWS);
    uint32_t* codes = R.out + TOP_OUT_HEAD;
    uint32_t g = 0, key[TS_MAX_WORDS];
    if (i < nrow) {
        g = codes[i];
        top_load(R.keys + (size_t)g * nw, nw, key);
#pragma unroll
        for (uint32_t j = 0; j < TS_MAX_WORDS; j++) pk[i * TS_MAX_WORDS + j] = key[j];
    }
    __syncthreads();                                               // (every code is read before any is written)
    if (i == 0) R.out[0] = nrow;
    if (i >= nrow) return;
    uint32_t pos = 0;
    for (uint32_t x = 0; x < nrow; x++) pos += ts_cmp(pk + x * TS_MAX_WORDS, key, TS_MAX_WORDS) < 0 ? 1u : 0u;
    codes[pos] = g;
    uint32_t* slot = R.out + TOP_OUT_HEAD + INFX_POST_MAX_ROWS + (size_t)pos * TOP_SLOT_WORDS;
    uint32_t c[4], mx, mn; int64_t S[XS_MAX_LIMBS];
    top_slot(R, g, c, &mx, &mn, S);
#pragma unroll
    for (int k = 0; k < 4; k++) slot[k] = c[k];
    slot[4] = mx; slot[5] = mn;
#pragma unroll
    for (int k = 0; k < XS_MAX_LIMBS; k++) { slot[STS_HEAD + 2 * k] = (uint32_t)(uint64_t)S[k]; slot[STS_HEAD + 2 * k + 1] = (uint32_t)((uint64_t)S[k] >> 32); }
}
