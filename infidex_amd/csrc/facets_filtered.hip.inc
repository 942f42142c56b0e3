// Facets of the documents a filter accepts, for up to INFX_MAX_PREFILTERS filters in ONE pass over the columns (infx_facets_filtered).
// Included by infidex_hip.hip after browse.hip.inc.  Not in the reference: the facet side of Query.pre_filter.
//
// k_facets_filtered is k_filter_mask_multi's walk (four consecutive documents per thread, a column's codes as one 16-byte load, the codes the programs
// read in the thread's LDS slots, the K programs one after another with wave-uniform control flow) with k_facets_all's counters behind it: instead of
// writing a mask, a document keeps its K-bit accept word in a register (bit k: not Deleted and program k accepts the document's OWN fields, as
// NumberOfDocumentsInFilter counts), and for every facet column c and every set bit k the counter [k][c][code] gets +1.
//   - a facet column that a program reads is taken from the thread's LDS slots (F.slot[c]); one that no program reads is loaded, once, when it is counted;
//   - a column the host placed in LDS (F.ldsOff[c] != ~0) is counted in per-workgroup LDS counters, K * nvals[c] words, merged with one global atomic
//     per (workgroup, counter that is not zero); any other column adds to its global counters directly;
//   - totals[k] += live accepted documents: ballot + popcount per wave, an LDS counter per workgroup, one global atomic per (workgroup, program).
// Integer atomics only, no position is decided by one: the sums do not depend on the order, on the placement or on the grid.
// Dynamic LDS: (nUsed * 4 * blockDim.x + K + ldsWords) words — codes lane-fastest as in k_filter_mask_multi, the program totals, the facet counters.
// out: program-major, out[k * stride + F.outOff[c] + code], stride = the sum of the facet columns' num_values.
struct DevFacetFilt {
    const uint32_t* codes[INFX_MAX_FACET_COLS]; uint32_t nvals[INFX_MAX_FACET_COLS]; uint32_t outOff[INFX_MAX_FACET_COLS];
    uint32_t ldsOff[INFX_MAX_FACET_COLS];      // 0xFFFFFFFF: global counters
    uint8_t slot[INFX_MAX_FACET_COLS];         // the column's slot among the codes the programs read (DevCountCols), 0xFF: no program reads it
};
#define FFL_BIG_THREADS 1024      // launches whose LDS counters exceed 16 KiB: one large workgroup per CU-sized share of LDS (infx_facets_filtered)
__global__ __launch_bounds__(FFL_BIG_THREADS) void k_facets_filtered(const DevFilter* __restrict__ progs, uint32_t K, DevCountCols cc, DevColumns cols, int32_t n,
                                                                  const uint8_t* __restrict__ deleted, DevFacetFilt F, int ncol, uint32_t ldsWords, uint32_t stride,
                                                                  uint32_t* __restrict__ out, uint32_t* __restrict__ totals) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ffl_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    uint32_t* codes = ffl_lds;                               // the thread's codes (filt_group4)
    uint32_t* cnt = ffl_lds + (size_t)cc.nUsed * 4u * T;     // [K] live accepted documents of this workgroup
    uint32_t* fac = cnt + K;                                 // [ldsWords] facet counters: F.ldsOff[c] + k * nvals[c] + code
    for (uint32_t i = tid; i < K + ldsWords; i += T) cnt[i] = 0;
    __syncthreads();
    const int64_t groups = ((int64_t)n + 3) >> 2;
    for (int64_t gb = (int64_t)blockIdx.x * T; gb < groups; gb += (int64_t)gridDim.x * T) {
        const FiltGroup4 g = filt_group4(gb + tid, groups, n, deleted, cc, cols, codes, tid, T);
        uint32_t acc[4] = {0, 0, 0, 0};                      // document j: bit k = program k accepts it and it is live
        for (uint32_t k = 0; k < K; k++) {
            const DevFilter f = progs[k];
            uint32_t hits = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool a = filt_eval_codes(f, [&](uint32_t c) { return codes[((uint32_t)cc.slot[c] * 4u + j) * T + tid]; });
                const bool hit = a && !((g.dead >> (8 * j)) & 0xFFu);
                hits += (uint32_t)__popcll(__ballot(hit));
                acc[j] |= (hit ? 1u : 0u) << k;
            }
            if ((tid & (WAVE - 1)) == 0 && hits) atomicAdd(&cnt[k], hits);
        }
        if (!__ballot((acc[0] | acc[1] | acc[2] | acc[3]) != 0)) continue;      // no document of this wave's 256 is in any filter: nothing to count (wave-uniform)
        for (int c = 0; c < ncol; c++) {
            const uint32_t nv = F.nvals[c];
            uint4 v;
            if (F.slot[c] != 0xFFu) { const uint32_t* cu = codes + (size_t)F.slot[c] * 4u * T + tid; v = make_uint4(cu[0], cu[T], cu[2 * T], cu[3 * T]); }
            else v = g.load4(F.codes[c], n);
            const uint32_t vj[4] = {v.x, v.y, v.z, v.w};
            const bool inLds = F.ldsOff[c] != 0xFFFFFFFFu;
            uint32_t* ctr = inLds ? fac + F.ldsOff[c] : out + F.outOff[c];
            const uint32_t step = inLds ? nv : stride;       // distance between two programs' counters of one value
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t w = vj[j] < nv ? acc[j] : 0u;       // (a dead document's accept word is 0)
                while (w) {
                    const uint32_t k = (uint32_t)__builtin_ctz(w); w &= w - 1;
                    atomicAdd(ctr + (size_t)k * step + vj[j], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < K; k += T) if (cnt[k]) atomicAdd(&totals[k], cnt[k]);
    for (int c = 0; c < ncol; c++) if (F.ldsOff[c] != 0xFFFFFFFFu) {
        const uint32_t nv = F.nvals[c];
        for (uint32_t i = tid; i < K * nv; i += T) {
            const uint32_t x = fac[F.ldsOff[c] + i];
            if (x) { const uint32_t k = i / nv, v = i - k * nv; atomicAdd(out + (size_t)k * stride + F.outOff[c] + v, x); }
        }
    }
}
