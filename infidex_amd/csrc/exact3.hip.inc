// Exact Stage-1 replay, parallel form (k_ex_walk x2 + k_ex_prefix -> k_ex_theta -> k_ex_chunk<1|4|16> -> k_ex_heap).  Same semantics as k_exact1 (see
// exact1.hip.inc for what is replayed and why); k_exact1 walks a query's chunks one after the other because a chunk's MaxScore skips need the heap
// threshold left by the chunks before it.  Here that chain is cut:
//   k_ex_walk   one wave per (flagged query, 65 536-id container), twice with k_ex_prefix in between: the candidate list C (arena rows that pass the tier
//               rule, ascending doc id), the candidates' first-pass scores side by side, the number of candidates up to every container's end.
//   k_ex_theta  one wave per flagged query: streams the first-pass scores in doc order, keeps the top-`depth` of them as a sorted array in the wave's
//               registers (8 per lane), cuts C into the reference's chunks (containers, <= 4096 candidates) and records for every chunk the threshold
//               its skips would see IF scores were k_accumulate's.
//   k_ex_chunk  one wave / 4 waves / 16 waves per chunk (by size), all chunks of all flagged queries at once: the terms in Bm25Scorer order; per term the
//               match list (hit mask minus MaxScore skips against the PREDICTED threshold, exact running scores), a ballot bitmap per 64 candidates,
//               mc and the start of the scalar tail from the bitmaps, then the exact fp32 score updates.  Emits the chunk's candidates that can still
//               enter the heap, and the interval [lo, hi) of thresholds for which every skip decision it took holds.
//   k_ex_heap   one wave per flagged query: UpdateTopK over the emitted candidates in doc order on the BCL 4-ary heap (in LDS while it fills, in registers
//               once full); before each chunk it checks that the EXACT threshold lies inside the chunk's interval.  If it does for every chunk, the
//               replay is the reference's computation bit for bit; if not (the predicted and the exact threshold straddle a skip bound: rare), the
//               query is handed to k_exact1.
#define EXS_MAXDEPTH 512          // sorted top-`depth` array of k_ex_theta: 8 registers x 64 lanes
#define EXC_SMALL 4               // tiles (64 candidates) per chunk handled by one wave            (k_ex_chunk<1>)
#define EXC_MID 16                //                                     by a 4-wave workgroup      (k_ex_chunk<4>)
#define EXC_BIG 64                // EX_CHUNK / 64:                      by a 16-wave workgroup     (k_ex_chunk<16>)
#define EXP_GRID1 8192            // workgroups of the k_ex_chunk<1> / <4> / <16> launches (grid-stride over the task lists)
#define EXP_GRID4 2048
#define EXP_GRID16 512
#define EXP_WORDS 16              // INFX_EXACT_PROF: u64 words per query (k_ex_heap 0..4, k_ex_theta 5..11)

struct ExChunk {                  // one reference chunk of one query
    uint32_t q, i0, n, full;      // query, first candidate (index into the query's candidate list), candidates, heap full at chunk start
    float theta;                  // predicted threshold at chunk start (0 while the heap is filling: exact)
    float lo, hi;                 // k_ex_chunk: every skip decision holds for thresholds in [lo, hi)
    uint32_t cnt;                 // k_ex_chunk: candidates emitted at out[i0 .. i0 + cnt)
};
struct ExQuery { uint32_t chunk0, nChunks, nCand, pad; };      // k_ex_theta: the query's chunks are exChunks[chunk0 .. +nChunks)

struct ExBufs {
    uint32_t* cand;               // per flagged query: candidate list = arena row indices relative to qBase[q], at cand[qBase[q] + i]
    infx_hit* out;                // k_ex_chunk output rows {local doc, exact score}, at out[qBase[q] + i0 + k]; between k_ex_walk<true> and k_ex_theta: the
                                  // first-pass score of candidate i in out[qBase[q] + i].score
    uint32_t* exc;                // per arena row: up to two (term + 1) << 8 | tf records (low / high half) for postings with tf >= 3
    ExChunk* chunks; uint32_t chunkCap;
    ExQuery* queries;             // nq
    uint32_t* counters;           // [0] chunks allocated, [1] one-wave tasks, [2] 4-wave tasks, [3] overflow flag, [4] 16-wave tasks
    uint32_t* tasksSmall; uint32_t* tasksMid; uint32_t* tasksBig;     // chunk indices
    uint32_t* contEnd;            // k_ex_walk / k_ex_prefix: per (query, container) the number of candidates in containers <= it (contEnd[q * nCont + c])
    unsigned long long* prof; unsigned long long* profChunk;      // INFX_EXACT_PROF (else nullptr): EXP_WORDS counters per query; 4 counters per k_ex_chunk workgroup
};

__device__ __forceinline__ float exs_wave_sum_f(float v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d); return v; }
__device__ __forceinline__ uint32_t exs_wave_sum_u(uint32_t v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d); return v; }

#define EXS_THREADS 256
// The candidate list of a flagged query — its arena rows that pass the tier rule, in doc order — is built by TWO sweeps of one wave per (query,
// 65 536-id container) with a per-query prefix in between:
//   k_ex_walk<false>  counts the container's passing rows                          -> contEnd[q][c]
//   k_ex_prefix       inclusive prefix over the containers of a query             -> contEnd[q][c] = candidates in containers <= c, queries[q].nCand
//   k_ex_walk<true>   the same walk, ballot-compacted behind the containers before: cand[] (arena row index) and the first-pass score side by side
// The rows of a container are its ranges' directory blocks (rows of a (query, range) are contiguous and ascend by doc id).  Measured (1000-query batch, 10 M
// documents, ~570 flagged queries): a query holds 70 k rows on average and up to 1.6 M (of which 20 k / 215 k pass); ONE workgroup per query walking them
// container by container (round 4's k_ex_scan, 5.0 ms) or directory segment by segment (8.9 ms with the threshold insertions split off) is bounded by those
// few queries — 87 k waves of ~460 rows are not.
template <bool WRITE>
__global__ __launch_bounds__(WAVE) void k_ex_walk(DevIndex ix, Arena ar, const SelRule* __restrict__ rules, const uint32_t* __restrict__ flagged, ExBufs xb, int nCont) {
    // ONE WAVE per (query, container), no barriers: the container's <= 128 directory entries sit two per lane; its ranges are walked one after the other (a range's rows
    // are contiguous: 64 per step, coalesced), the loads of the next range in flight while the current one is counted / compacted by ballots.
    const int q = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    if (flagged[q] != 1u) return;
    const SelRule rule = rules[q];
    const unsigned long long qb = ar.qBase[q];
    const int rsh = 16 - ix.rshift, rpc = 1 << rsh;             // ranges per container (R <= 16384, R >= 512: 4 .. 128)
    const int r0 = c << rsh, nr = min(ix.nRanges - r0, rpc);
    const uint2* dir = ar.dir + (unsigned long long)q * ix.nRanges + r0;
    uint2 e0 = make_uint2(0u, 0u), e1 = make_uint2(0u, 0u);     // entries lane and lane + 64: {arena offset, rows}
    if (lane < nr) e0 = dir[lane];
    if (lane + WAVE < nr) e1 = dir[lane + WAVE];
    unsigned long long live0 = __ballot(e0.y != 0u), live1 = __ballot(e1.y != 0u);
    uint32_t* cand = nullptr; infx_hit* sc0 = nullptr; uint32_t nPass = 0;
    if (WRITE) { cand = xb.cand + qb; sc0 = xb.out + qb; nPass = c > 0 ? xb.contEnd[(size_t)q * nCont + c - 1] : 0u; }
    uint32_t count = 0;
    const unsigned long long lt = (1ull << lane) - 1;
    for (int half = 0; half < 2; half++) {
        unsigned long long live = half ? live1 : live0;
        const uint2 e = half ? e1 : e0;
        while (live) {
            const int k = __ffsll((long long)live) - 1; live &= live - 1;
            const uint32_t off = rdl_u(e.x, k), n = rdl_u(e.y, k);
            for (uint32_t v0 = 0; v0 < n; v0 += WAVE) {
                const uint32_t v = v0 + lane; const bool in = v < n;
                const uint32_t rowRel = off + v;
                const uint8_t cls = in ? ar.cls[qb + rowRel] : (uint8_t)0;
                float sc = 0.f; if (WRITE && in) sc = ar.score[qb + rowRel];
                const bool pass = in && sel_pass(rule, cls);
                const unsigned long long bp = __ballot(pass);
                if (WRITE && pass) { const uint32_t pidx = nPass + (uint32_t)__popcll(bp & lt); cand[pidx] = rowRel; sc0[pidx].score = sc; }
                const uint32_t np = (uint32_t)__popcll(bp);
                nPass += np; count += np;
            }
        }
    }
    if (!WRITE && lane == 0) xb.contEnd[(size_t)q * nCont + c] = count;
}
__global__ __launch_bounds__(EXS_THREADS) void k_ex_prefix(const uint32_t* __restrict__ flagged, ExBufs xb, int nCont) {
    __shared__ uint32_t sWave[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (flagged[q] != 1u) return;
    uint32_t* ce = xb.contEnd + (size_t)q * nCont;
    uint32_t carry = 0;
    for (int c0 = 0; c0 < nCont; c0 += EXS_THREADS) {
        const uint32_t v = c0 + tid < nCont ? ce[c0 + tid] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if (lane >= d) incl += x; }
        __syncthreads();
        if (lane == WAVE - 1) sWave[wv] = incl;
        __syncthreads();
        uint32_t base = carry; for (int w = 0; w < wv; w++) base += sWave[w];
        if (c0 + tid < nCont) ce[c0 + tid] = base + incl;
        carry += sWave[0] + sWave[1] + sWave[2] + sWave[3];
    }
    if (tid == 0) { ExQuery Q; Q.chunk0 = 0; Q.nChunks = 0; Q.nCand = carry; Q.pad = 0; xb.queries[q] = Q; }
}

// k_ex_theta — one wave per flagged query, the sequential rest of the scan: the candidates' first-pass scores stream by in doc order (contiguous since
// k_ex_walk: 256 per step, the next step's loads in flight), every score above the running threshold is inserted into the sorted top-`depth` array
// (wave registers: element e in lane e / 8, register e % 8), and at every chunk boundary — a container's end or 4096 candidates — the chunk is recorded
// with the threshold its skips would see IF scores were k_accumulate's, and handed to the k_ex_chunk variant of its size.
//   * The first `depth` candidates need no insertion: none of them can be refused, and every boundary before the depth-th sees threshold 0.  They are
//     sorted in one go (bitonic, LDS) — a quarter of all insertions.
//   * An insertion is ~35 instructions and no LDS round trip: the position from eight ballots, the neighbour lane's last element by DPP wave_shr, and one
//     of eight straight-line shift sequences picked by the position's register (scalar branch).  (Round 4: ~920 cycles per insertion through ds_bpermute.)
// prior (document shards only, else nullptr): per query the top-`depth` first-pass scores of the shards BEFORE this one, descending, zero padded to
// EXS_MAXDEPTH (k_gflag) — the state a single index's scan would have reached at this shard's first document.
#define EXT_BLOCK 1024            // candidates per LDS block of k_ex_theta
#define EXT_CONT 512              // container ends held in LDS at a time
template <int IP> __device__ __forceinline__ void exs_shift_in(float (&s)[8], float x, float prev7, bool gt, bool eq) {
    // elements behind position (lane lp, register IP) move one place down, x lands there.  gt: lane > lp, eq: lane == lp
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const float src = i > 0 ? s[i - 1] : prev7;
        if (i > IP) s[i] = (gt || eq) ? src : s[i];
        else if (i == IP) s[i] = gt ? src : (eq ? x : s[i]);
        else s[i] = gt ? src : s[i];
    }
}
__global__ __launch_bounds__(WAVE) void k_ex_theta(Arena ar, const SelRule* __restrict__ rules, uint32_t* __restrict__ flagged, ExBufs xb, const float* __restrict__ prior, int nCont) {
    __shared__ float sSort[EXS_MAXDEPTH], sBlock[EXT_BLOCK]; __shared__ uint32_t sCont[EXT_CONT];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (flagged[q] != 1u) return;
    long long pT = 0, pIns = 0; unsigned long long nIns = 0; if (xb.prof) pT = (long long)__builtin_readcyclecounter();
    const int depth = rules[q].depth;
    const unsigned long long qb = ar.qBase[q];
    const uint32_t nCand = xb.queries[q].nCand;
    const infx_hit* sc0 = xb.out + qb;
    const uint32_t* contEnd = xb.contEnd + (size_t)q * nCont;
    uint32_t chunk0;
    {   const uint32_t maxChunks = (uint32_t)nCont + nCand / EX_CHUNK + 2u;
        uint32_t c0 = 0; if (lane == 0) { c0 = atomicAdd(&xb.counters[0], maxChunks); if (c0 + maxChunks > xb.chunkCap) { atomicExch(&xb.counters[3], 1u); c0 = 0xFFFFFFFFu; } }
        chunk0 = rdl_u(c0, 0); }
    if (chunk0 == 0xFFFFFFFFu) { if (lane == 0) flagged[q] = 2u; return; }          // cannot happen with the host's sizing; k_exact1 would still be right
    // ---- top-`depth` device scores so far, descending; element e lives in lane e / 8, register e % 8 ---------------------------------------------
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = prior ? prior[(size_t)q * EXS_MAXDEPTH + 8 * lane + i] : 0.f;
    const int thLane = (depth - 1) >> 3, thReg = (depth - 1) & 7;
    auto theta_now = [&]() -> float {                      // element depth-1 (0 while fewer than depth scores were inserted).  Every register is read at a
        const float v0 = rdl_f(s[0], thLane), v1 = rdl_f(s[1], thLane), v2 = rdl_f(s[2], thLane), v3 = rdl_f(s[3], thLane);     // constant index: a select
        const float v4 = rdl_f(s[4], thLane), v5 = rdl_f(s[5], thLane), v6 = rdl_f(s[6], thLane), v7 = rdl_f(s[7], thLane);     // over s[] by register number
        const float lo4 = thReg == 0 ? v0 : (thReg == 1 ? v1 : (thReg == 2 ? v2 : v3));                                          // turns into a dynamically
        const float hi4 = thReg == 4 ? v4 : (thReg == 5 ? v5 : (thReg == 6 ? v6 : v7));                                          // indexed array in scratch
        return thReg < 4 ? lo4 : hi4;
    };
    auto insert = [&](const float x) {                     // x wave-uniform
        // position p = elements strictly greater than x.  The array is sorted, so the lanes whose LAST element is greater hold only greater elements (one
        // ballot); the boundary lane's own count comes from eight VALU compares accumulated with carry-adds and one v_readlane — instead of eight ballots,
        // each a VALU -> SALU hand-over the scalar unit waits for.
        const int lp = __popcll(__ballot(s[7] > x));       // lanes 0 .. lp-1 are entirely greater (lp == 64: x is below everything)
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) cnt += s[i] > x ? 1u : 0u;
        const int p = lp < WAVE ? 8 * lp + (int)rdl_u(cnt, lp) : 8 * WAVE;
        if (p >= depth) return;
        const float prev7 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s[7]), 0x138 /* wave_shr:1 */, 0xF, 0xF, false));
        const bool gt = lane > lp, eq = lane == lp;
        switch (p & 7) {
            case 0: exs_shift_in<0>(s, x, prev7, gt, eq); break; case 1: exs_shift_in<1>(s, x, prev7, gt, eq); break;
            case 2: exs_shift_in<2>(s, x, prev7, gt, eq); break; case 3: exs_shift_in<3>(s, x, prev7, gt, eq); break;
            case 4: exs_shift_in<4>(s, x, prev7, gt, eq); break; case 5: exs_shift_in<5>(s, x, prev7, gt, eq); break;
            case 6: exs_shift_in<6>(s, x, prev7, gt, eq); break; default: exs_shift_in<7>(s, x, prev7, gt, eq); break;
        }
    };
    uint32_t nChunks = 0, cStart = 0; float cTheta = theta_now();
    auto close_chunk = [&](uint32_t endIdx) {              // candidates [cStart, endIdx); every score before endIdx has been inserted
        if (endIdx > cStart) {
            if (lane == 0) {
                // "heap full at chunk start" is predicted from the first-pass scores: `depth` positive scores seen so far (deleted documents carry score 0
                // and are never offered to the heap; k_ex_heap verifies the prediction)
                ExChunk c; c.q = (uint32_t)q; c.i0 = cStart; c.n = endIdx - cStart; c.full = cTheta > 0.f ? 1u : 0u; c.theta = cTheta; c.lo = 0.f; c.hi = 0.f; c.cnt = 0;
                xb.chunks[chunk0 + nChunks] = c;
                const uint32_t tiles = (c.n + 63u) / 64u;
                if (tiles <= EXC_SMALL) xb.tasksSmall[atomicAdd(&xb.counters[1], 1u)] = chunk0 + nChunks;
                else if (tiles <= EXC_MID) xb.tasksMid[atomicAdd(&xb.counters[2], 1u)] = chunk0 + nChunks;
                else xb.tasksBig[atomicAdd(&xb.counters[4], 1u)] = chunk0 + nChunks;
            }
            nChunks++;
        }
        cStart = endIdx;
        cTheta = theta_now();                               // predicted threshold at the start of the next chunk
    };
    // chunk boundaries: the next one is the end of the current container (the first whose end lies beyond cStart) or cStart + 4096.  The container ends
    // sit in LDS (EXT_CONT at a time): a global load here would make the compiler wait for the score prefetch of the next block as well
    int cc = 0, ccBase = 0;
    auto load_cont = [&](int base) { for (int i = lane; i < EXT_CONT; i += WAVE) sCont[i] = base + i < nCont ? contEnd[base + i] : nCand; __builtin_amdgcn_wave_barrier(); };
    load_cont(0);
    auto next_boundary = [&]() -> uint32_t {
        for (;;) {
            if (cc >= nCont) break;
            if (cc - ccBase >= EXT_CONT) { ccBase = cc; load_cont(ccBase); }
            if (rfl_i((int)sCont[cc - ccBase]) > (int)cStart) break;
            cc++;
        }
        const uint32_t ce = cc < nCont ? (uint32_t)rfl_i((int)sCont[cc - ccBase]) : nCand;
        return min(ce, cStart + (uint32_t)EX_CHUNK);
    };
    uint32_t nb = nCand ? next_boundary() : 0u;
    // ---- the first `depth` candidates in one go (single index only: a shard starts from the state of the shards before it) ---------------------------
    uint32_t done = 0;                                      // candidates [0, done) are in the array
    if (!prior && depth >= 64) {
        const uint32_t B = min(nCand, (uint32_t)depth);
        while (nb < B) { close_chunk(nb); nb = next_boundary(); }          // boundaries before the depth-th candidate: threshold 0 (s is still all zeros)
        for (int i = lane; i < EXS_MAXDEPTH; i += WAVE) sSort[i] = (uint32_t)i < B ? sc0[i].score : 0.f;
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int k = 2; k <= EXS_MAXDEPTH; k <<= 1)
#pragma unroll 1
            for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
                for (int u = 0; u < EXS_MAXDEPTH / 2 / WAVE; u++) {
                    const int t = u * WAVE + lane;                           // pair t: elements a = insert a zero bit at position log2(j), b = a | j
                    const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                    const float va = sSort[a], vb = sSort[b];
                    const bool desc = (a & k) == 0;                          // descending overall
                    if (desc ? (va < vb) : (va > vb)) { sSort[a] = vb; sSort[b] = va; }
                }
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
        for (int i = 0; i < 8; i++) s[i] = sSort[8 * lane + i];
        done = B;
    }
    // ---- the stream: blocks of EXT_BLOCK candidates through LDS; the next block's loads (EXT_BLOCK / 64 per lane) are in flight while this one is processed --
    float th = theta_now();                                 // insert prefilter: the current threshold, refreshed after every insertion
    float nxt[EXT_BLOCK / WAVE];
    const uint32_t tBeg = done & ~(uint32_t)(EXT_BLOCK - 1);
#pragma unroll
    for (int k = 0; k < EXT_BLOCK / WAVE; k++) { const uint32_t i = tBeg + (uint32_t)k * WAVE + lane; nxt[k] = i < nCand ? sc0[i].score : 0.f; }
    for (uint32_t t0 = tBeg; t0 < nCand; t0 += EXT_BLOCK) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < EXT_BLOCK / WAVE; k++) sBlock[k * WAVE + lane] = nxt[k];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < EXT_BLOCK / WAVE; k++) { const uint32_t i = t0 + EXT_BLOCK + (uint32_t)k * WAVE + lane; nxt[k] = i < nCand ? sc0[i].score : 0.f; }
        const int nt = (int)((min(nCand - t0, (uint32_t)EXT_BLOCK) + WAVE - 1) / WAVE);
        float vnext = sBlock[lane];
#pragma unroll 1
        for (int k = 0; k < nt; k++) {
            const uint32_t t = t0 + (uint32_t)k * WAVE;
            const float v = vnext;
            if (k + 1 < nt) vnext = sBlock[(k + 1) * WAVE + lane];
            if (t + WAVE <= done) continue;
            unsigned long long w = __ballot(t + lane >= done && t + lane < nCand && v > th);
            if (w) {
                if (xb.prof) { nIns += (unsigned long long)__popcll(w); pIns -= (long long)__builtin_readcyclecounter(); }
                do {
                    const int b = __ffsll((long long)w) - 1; w &= w - 1;
                    while (t + (uint32_t)b >= nb) { close_chunk(nb); nb = next_boundary(); }
                    insert(rdl_f(v, b));
                } while (w);
                th = theta_now();
                if (xb.prof) pIns += (long long)__builtin_readcyclecounter();
            }
            while (min(t + (uint32_t)WAVE, nCand) >= nb && cStart < nCand) { close_chunk(nb); if (cStart < nCand) nb = next_boundary(); }
        }
    }
    while (cStart < nCand) { close_chunk(nb); if (cStart < nCand) nb = next_boundary(); }      // (every candidate went in with the first `depth`: no tile closed them)
    if (lane == 0) {
        ExQuery Q; Q.chunk0 = chunk0; Q.nChunks = nChunks; Q.nCand = nCand; Q.pad = 0; xb.queries[q] = Q;
        if (xb.prof) { unsigned long long* P = xb.prof + (size_t)q * EXP_WORDS; P[11] = (unsigned long long)((long long)__builtin_readcyclecounter() - pT); P[5] = P[11]; P[6] = (unsigned long long)pIns; P[7] = nIns; P[10] = nCand; }
    }
}

// tf of a posting whose mask code is 3 (tf >= 3): from the row's exception record, else from the posting list
__device__ __forceinline__ float ex_tf3(const DevIndex& ix, uint32_t exc, int t, int32_t termId, int32_t doc) {
    if (((exc >> 8) & 0x7Fu) == (uint32_t)(t + 1)) return (float)(exc & 0xFFu);
    if (((exc >> 24) & 0x7Fu) == (uint32_t)(t + 1)) return (float)((exc >> 16) & 0xFFu);
    return ex_tf_lookup(ix, termId, doc);
}

// k_ex_chunk<W>: grid-stride over a task list; W waves per chunk (1: chunks of <= 4 tiles of 64 candidates, 4: <= 16 tiles, 16: <= 64 tiles = 4096
// candidates).  Tile k belongs to wave k % W, slot k / W: every lane keeps its <= 4 candidates — hit masks, doc id, norm, running exact score — in
// registers for the whole term loop.  Per term: (a) the match ballots of the wave's tiles, (b) W > 1: the ballot words meet in LDS (one barrier per
// term, double buffered), every wave derives the match count and the start of the scalar tail from them on its own, (c) the exact score updates.
// (Round 4's chunks of more than 4 tiles ran on ONE wave with two to four dependent global loads per (term, tile): 2.3 ms per batch for the two launches.)
template <int W>
__global__ __launch_bounds__(W * WAVE) void k_ex_chunk(DevIndex ix, const DevQuery* __restrict__ queries, const DevRefTerm* __restrict__ refTerms, Arena ar, ExBufs xb,
                                                        const uint32_t* __restrict__ tasks, int taskCounter, float avgdlIn) {
    constexpr int NT = W * 4;                              // tiles a workgroup can hold
    __shared__ unsigned long long sBal[2][NT];
    __shared__ uint32_t sEmit[NT]; __shared__ float sLo[W], sHi[W];
    const int lane = threadIdx.x & 63, wv = W > 1 ? (int)(threadIdx.x >> 6) : 0;
    const int MW = ar.maskWords;
    const uint32_t nTasks = xb.counters[taskCounter];
    const float avgdl = avgdlIn > 0.f ? avgdlIn : 1.f;
    for (uint32_t task = blockIdx.x; task < nTasks; task += gridDim.x) {
        long long pT = 0; if (xb.profChunk) pT = (long long)__builtin_readcyclecounter();      // per-workgroup slots, plain stores: atomics on shared counters serialise at L2 and distort what they measure
        const uint32_t ci = tasks[task];
        const ExChunk C = xb.chunks[ci];
        const int q = (int)C.q;
        const DevQuery Q = queries[q];
        const int nRef = (int)Q.numRef;
        const DevRefTerm* RT = refTerms + Q.refOff;
        const unsigned long long qb = ar.qBase[q];
        const uint32_t* cand = xb.cand + qb + C.i0;
        const int n = (int)C.n, T = (n + WAVE - 1) / WAVE;
        const float th = C.full ? C.theta : 0.f;
        // the query's reference terms, one per lane (nRef <= 64 whenever the replay runs), and their suffix sums (ComputeSuffixSums :524-533, in its fp32
        // order), element i in lane i
        DevRefTerm myRT; myRT.idf = 0.f; myRT.maxScore = 0.f; myRT.termId = -1; myRT.unit = 0;
        if (lane < nRef) myRT = RT[lane];
        float mySuf = 0.f;
        { float run = 0.f; for (int i = nRef - 1; i >= 0; i--) { run = run + rdl_f(myRT.maxScore, i); if (lane == i) mySuf = run; } }
        unsigned long long rM0[4], rM1[4]; int32_t rDoc[4]; float rNorm[4], rCur[4]; uint32_t rRow[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            rM0[i] = 0; rM1[i] = 0; rDoc[i] = 0; rNorm[i] = 1.f; rCur[i] = 0.f; rRow[i] = 0;
            const int k = i * W + wv, j = k * WAVE + lane;
            if (k < T && j < n) {
                rRow[i] = cand[j];
                const unsigned long long row = qb + rRow[i];
                rM0[i] = ar.mask[row * (unsigned long long)MW]; if (MW > 1) rM1[i] = ar.mask[row * (unsigned long long)MW + 1];
                rDoc[i] = ar.doc[row] - ix.docBase; rNorm[i] = ix.docNorm[rDoc[i]];
            }
        }
        float lo = 0.f, hi = __builtin_inff();              // skip decisions hold for thresholds in [lo, hi)
        int buf = 0;
        for (int t = 0; t < nRef; t++) {
            DevRefTerm rt; rt.idf = rdl_f(myRT.idf, t); rt.maxScore = rdl_f(myRT.maxScore, t); rt.termId = __builtin_amdgcn_readlane(myRT.termId, t); rt.unit = rdl_u(myRT.unit, t);
            if (!(rt.idf > 0.f)) continue;                  // :301-309
            const float ms = rt.maxScore, rem = t + 1 < nRef ? rdl_f(mySuf, t + 1) : 0.f;
            const int wsel = t >> 5, sh = (t & 31) * 2;
            // (a) match list: hit and not skipped; one ballot word per 64 candidates — ballots are scalar values, so the match count and the start of
            // the scalar tail are computed on the scalar unit
            unsigned long long balk[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = i * W + wv, j = k * WAVE + lane;
                bool match = false;
                if (k < T && j < n) {
                    const unsigned long long m = wsel ? rM1[i] : rM0[i];
                    if ((m >> sh) & 3ull) {
                        const float bound = (rCur[i] + ms) + rem;                           // :350-368
                        if (bound <= th) lo = fmaxf(lo, bound); else { match = true; hi = fminf(hi, bound); }
                    }
                }
                balk[i] = __ballot(match);
            }
            uint32_t mc = 0; int tailTile = T, tailBit = 0;     // candidates (tile, bit) >= (tailTile, tailBit) are in the scalar tail: the last mc % 8 matches (:395-444)
            if (W == 1) {
#pragma unroll
                for (int i = 0; i < 4; i++) mc += (uint32_t)__popcll(balk[i]);
                if (mc == 0) continue;
                uint32_t need = mc & 7u;
                if (need) {
#pragma unroll
                    for (int k = 3; k >= 0; k--) {
                        if (k >= T || tailTile != T) continue;
                        const uint32_t c = (uint32_t)__popcll(balk[k]);
                        if (c >= need) {
                            unsigned long long w = balk[k];
                            for (uint32_t x = 1; x < need; x++) w &= ~(1ull << (63 - __clzll((long long)w)));
                            tailTile = k; tailBit = 63 - __clzll((long long)w);
                        } else need -= c;
                    }
                }
            } else {
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 4; i++) sBal[buf][i * W + wv] = balk[i];
                }
                __syncthreads();
                const unsigned long long wk = lane < T ? sBal[buf][lane] : 0ull;     // tile `lane`'s word (T <= NT <= 64)
                buf ^= 1;
                const uint32_t mcLane = (uint32_t)__popcll(wk);
                uint32_t incl = mcLane;                      // inclusive prefix over lanes (tiles)
#pragma unroll
                for (int d = 1; d < WAVE; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if (lane >= d) incl += x; }
                mc = rdl_u(incl, WAVE - 1);
                if (mc == 0) continue;
                const uint32_t r = mc & 7u;
                if (r) {
                    const uint32_t after = mc - incl;            // matches in tiles after mine
                    const bool here = lane < T && after < r && after + mcLane >= r;     // the r-th match from the end lies in my tile
                    const unsigned long long hb = __ballot(here);
                    const int kt = __ffsll((long long)hb) - 1;
                    const uint32_t need = r - rdl_u(after, kt);          // the need-th set bit from the top of tile kt's word
                    unsigned long long w = rfl_u64(__shfl(wk, kt));
                    for (uint32_t x = 1; x < need; x++) w &= ~(1ull << (63 - __clzll((long long)w)));
                    tailTile = kt; tailBit = 63 - __clzll((long long)w);
                }
            }
            // (c) exact score updates
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = i * W + wv;
                if (!((balk[i] >> lane) & 1ull)) continue;
                const uint32_t code = (uint32_t)(((wsel ? rM1[i] : rM0[i]) >> sh) & 3ull);
                const int32_t doc = rDoc[i];
                const float tf = (rt.unit || code == 1u) ? 1.0f : (code == 2u ? 2.0f : ex_tf3(ix, xb.exc[qb + rRow[i]], t, rt.termId, doc));
                float sc;
                const bool tail = k > tailTile || (k == tailTile && lane >= tailBit);
                if (!tail) {
                    const float denom = tf + rNorm[i];                                // Vector256 lanes: K1 * ((1-B) + (B/avgdl) * dl)
                    const float core = (tf * (1.2f + 1.0f)) / denom;
                    sc = rt.idf * (core + 1.0f);
                } else {                                                                // ComputeTermScore :643-652
                    float dl = ix.docLen[doc]; if (dl <= 0.f) dl = 1.f;
                    const float normFactor = 1.2f * (1.f - 0.75f + 0.75f * (dl / avgdl));
                    const float denom = tf + normFactor;
                    if (denom <= 0.f) sc = 0.f;
                    else { const float core = (tf * (1.2f + 1.f)) / denom; sc = rt.idf * (core + 1.0f); }
                }
                rCur[i] += sc;
            }
        }
        // emit, in chunk order, the candidates UpdateTopK could still accept (the exact threshold is >= the predicted one up to a few ulp)
        const float keep = th * (1.0f - 1e-5f);
        infx_hit* out = xb.out + qb + C.i0;
        bool f[4]; int32_t gd[4]; unsigned long long eb[4];
        const uint8_t* del = q_deleted(ix, (uint32_t)q);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = i * W + wv, j = k * WAVE + lane;
            const float sv = (k < T && j < n) ? rCur[i] : 0.f;
            // a deleted document (Bm25Scorer.cs:322-323) is scored with its chunk (it holds its position in the match lists) but never reaches UpdateTopK
            gd[i] = rDoc[i] + ix.docBase;
            f[i] = sv > 0.f && (!C.full || sv > keep) && !(del && del[gd[i]]);
            eb[i] = __ballot(f[i]);
        }
        for (int d = 32; d > 0; d >>= 1) { lo = fmaxf(lo, __shfl_xor(lo, d)); hi = fminf(hi, __shfl_xor(hi, d)); }
        uint32_t cnt = 0;
        if (W == 1) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (f[i]) { infx_hit h; h.doc = gd[i]; h.score = rCur[i]; out[cnt + __popcll(eb[i] & ((1ull << lane) - 1))] = h; }
                cnt += (uint32_t)__popcll(eb[i]);
            }
        } else {
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 4; i++) sEmit[i * W + wv] = (uint32_t)__popcll(eb[i]);
                sLo[wv] = lo; sHi[wv] = hi;
            }
            __syncthreads();
            const uint32_t ck = lane < NT ? sEmit[lane] : 0u;
            uint32_t incl = ck;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if (lane >= d) incl += x; }
            cnt = rdl_u(incl, WAVE - 1);
            const uint32_t excl = incl - ck;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t base = rdl_u(excl, i * W + wv);
                if (f[i]) { infx_hit h; h.doc = gd[i]; h.score = rCur[i]; out[base + __popcll(eb[i] & ((1ull << lane) - 1))] = h; }
            }
            for (int w = 0; w < W; w++) { lo = fmaxf(lo, sLo[w]); hi = fminf(hi, sHi[w]); }
        }
        if (threadIdx.x == 0) {
            xb.chunks[ci].cnt = cnt; xb.chunks[ci].lo = lo; xb.chunks[ci].hi = hi;
            if (xb.profChunk) { const unsigned long long cy = (unsigned long long)((long long)__builtin_readcyclecounter() - pT);
                                unsigned long long* P = xb.profChunk + ((W == 1 ? 0 : (W == 4 ? EXP_GRID1 : EXP_GRID1 + EXP_GRID4)) + blockIdx.x) * 4;
                                P[0] += 1ull; P[1] += cy; P[2] = P[2] > cy ? P[2] : cy; P[3] += (unsigned long long)T; }
        }
        if (W > 1) __syncthreads();                          // sEmit / sLo / sHi / sBal are reused by the next task
    }
}

// PriorityQueue<int,float> (4-ary min-heap, BCL sift rules — see ExHeap) executed by a whole wave in lock step: nodes 0..63 (the top three
// levels and most of the fourth) live in registers, node i in lane i, read with v_readlane / written with a lane-select; deeper nodes live in
// LDS as packed {priority, doc} words read with one broadcast load per child.  A sift step near the root costs a few scalar-indexed
// register reads instead of an LDS round trip per level.
struct WHeap {                                // priorities are positive floats: kept and compared as their uint32 bit patterns (order preserving), so
    uint32_t rp; int32_t rd;                  // the sift logic runs on the scalar unit.  rp/rd: this lane's node (node index == lane)
    unsigned long long* lds;                  // every node: {priority bits, doc} (nodes < 64 are mirrored in the registers above)
    int n;
    __device__ __forceinline__ uint32_t getp(int i) const { return i < WAVE ? rdl_u(rp, i) : (uint32_t)rfl_i((int)(uint32_t)lds[i]); }
    __device__ __forceinline__ int32_t getd(int i) const { return i < WAVE ? __builtin_amdgcn_readlane(rd, i) : rfl_i((int)(uint32_t)(lds[i] >> 32)); }
    __device__ __forceinline__ void set(int i, uint32_t p, int32_t d) {
        if (i < WAVE) { const bool me = (int)threadIdx.x == i; rp = me ? p : rp; rd = me ? d : rd; }
        if (threadIdx.x == 0) lds[i] = ((unsigned long long)(uint32_t)d << 32) | p;
    }
    __device__ void move_up(uint32_t np, int32_t nd, int idx) {
        while (idx > 0) {
            const int parent = (idx - 1) >> 2;
            const uint32_t pp = getp(parent);
            if (np < pp) { set(idx, pp, getd(parent)); idx = parent; } else break;
        }
        set(idx, np, nd);
    }
    __device__ void move_down(uint32_t np, int32_t nd, int idx) {
        int i;
        while ((i = (idx << 2) + 1) < n) {
            // the four children in one step: register reads near the root, ONE LDS load (lanes 0..3) below it
            uint32_t c0, c1, c2, c3; int32_t d0, d1, d2, d3;
            if (i + 3 < WAVE) {
                c0 = rdl_u(rp, i); c1 = rdl_u(rp, i + 1); c2 = rdl_u(rp, i + 2); c3 = rdl_u(rp, i + 3);
                d0 = __builtin_amdgcn_readlane(rd, i); d1 = __builtin_amdgcn_readlane(rd, i + 1); d2 = __builtin_amdgcn_readlane(rd, i + 2); d3 = __builtin_amdgcn_readlane(rd, i + 3);
            } else {
                const int k = (int)(threadIdx.x & 3u);
                unsigned long long v = 0xFFFFFFFFull;
                if (threadIdx.x < 4 && i + k < n) v = lds[i + k];
                const uint32_t vp = (uint32_t)v; const int32_t vd = (int32_t)(uint32_t)(v >> 32);
                c0 = rdl_u(vp, 0); c1 = rdl_u(vp, 1); c2 = rdl_u(vp, 2); c3 = rdl_u(vp, 3);
                d0 = __builtin_amdgcn_readlane(vd, 0); d1 = __builtin_amdgcn_readlane(vd, 1); d2 = __builtin_amdgcn_readlane(vd, 2); d3 = __builtin_amdgcn_readlane(vd, 3);
            }
            if (i + 1 >= n) c1 = 0xFFFFFFFFu;
            if (i + 2 >= n) c2 = 0xFFFFFFFFu;
            if (i + 3 >= n) c3 = 0xFFFFFFFFu;
            uint32_t mp = c0; int mi = i; int32_t md = d0;      // first minimal child wins, as in the BCL loop
            if (c1 < mp) { mp = c1; mi = i + 1; md = d1; }
            if (c2 < mp) { mp = c2; mi = i + 2; md = d2; }
            if (c3 < mp) { mp = c3; mi = i + 3; md = d3; }
            if (np <= mp) break;
            set(idx, mp, md); idx = mi;
        }
        set(idx, np, nd);
    }
    __device__ void enqueue(int32_t nd, uint32_t np) { n++; move_up(np, nd, n - 1); }
    __device__ void enqueue_dequeue(int32_t nd, uint32_t np) { if (n > 0 && np > getp(0)) move_down(np, nd, 0); }
};

// ---- The FULL heap in registers (round 5) -----------------------------------------------------------------------------------------------------
// Once `depth` entries are in, UpdateTopK only ever calls EnqueueDequeue: the root leaves, the chain of first-minimal children moves up one level
// each until the new priority is <= the next one, the new entry takes the last vacated node.  WHeap pays an LDS round trip per level for that
// (1 000-2 000 cycles per operation, 3-4 k operations per query on one wave: 3.5 ms per batch).  Here the whole heap lives in the wave's registers:
//   * the four CHILDREN of a node sit in ONE lane (a "group"), kept sorted by (priority bits, sibling index) — entry 0 is the first minimal child
//     the BCL loop would pick, with its sibling index in the top two bits of the doc word (internal ids < 2^30: the host checks);
//   * group g (children of node g, nodes 4g+1 .. 4g+4) is placed so that every LEVEL has a fixed register: levels 1-3 (groups 0..20) in slot 0
//     lanes 0..20, level 4 (groups 21..84) in slot 1 lanes 0..63, level 5 (groups 85..127, depth <= 512) in slot 0 lanes 21..63;
//   * an operation is five straight scalar steps — v_readlane of the group's minimum (lane index from an SGPR), compare, v_writelane of that
//     minimum into the vacated lane's "pending" register — and one lane-local re-insertion of the pending entry per slot (3 compares, 12 selects).
// Nodes that do not exist carry priority 0xFFFFFFFF (every real priority is the bit pattern of a positive float): no bound checks.
#define RH_DOCM 0x3FFFFFFFu
#define RH_KM 0xC0000000u
// v_writelane_b32 (this clang has no builtin for it): value and lane select are wave-uniform.  gfx9 reads one SGPR per VALU instruction, so the lane
// select travels in M0 (the compiler reserves M0 and re-loads it before each of its own uses; it holds nothing across statements).  The ISA's manual
// hazard "lane select written by a VALU instruction: 4 wait states" does not arise: M0 is written by s_mov right before.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ uint32_t wrl_u(uint32_t old, uint32_t val, int l) {
    val = (uint32_t)rfl_i((int)val); l = rfl_i(l);      // both ARE uniform; this pins them to SGPRs where the compiler's divergence analysis cannot tell
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(old) : "s"(val), "s"(l) : "m0");
    return old;
}
// two pending registers of one lane in one go (one M0 load)
__device__ __forceinline__ void wrl2_u(uint32_t& r0, uint32_t v0, uint32_t& r1, uint32_t v1, int l) {
    v0 = (uint32_t)rfl_i((int)v0); v1 = (uint32_t)rfl_i((int)v1); l = rfl_i(l);
    asm volatile("s_mov_b32 m0, %4\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %3, m0" : "+v"(r0), "+v"(r1) : "s"(v0), "s"(v1), "s"(l) : "m0");
}
#pragma clang diagnostic pop
__device__ __forceinline__ bool rh_gt(uint32_t pa, uint32_t la, uint32_t pb, uint32_t lb) { return pa > pb || (pa == pb && la > lb); }
struct RHeap {
    uint32_t p0[4], l0[4], p1[4], l1[4];       // the lane's two groups, each sorted ascending by (priority bits, sibling index): l = sibling << 30 | doc
    uint32_t np0, nl0, np1, nl1;               // the entry that takes the place of the group's entry 0 at the next settle(); idle lanes hold their own entry 0
    uint32_t rootP; uint32_t rootD;            // node 0 (wave-uniform)
    __device__ __forceinline__ static int group0(int lane) { return lane < 21 ? lane : lane + 64; }
    __device__ __forceinline__ static int group1(int lane) { return lane + 21; }
    __device__ __forceinline__ static void cswap(uint32_t& pa, uint32_t& la, uint32_t& pb, uint32_t& lb) {
        const bool g = rh_gt(pa, la, pb, lb);
        const uint32_t tp = g ? pb : pa, tl = g ? lb : la; pb = g ? pa : pb; lb = g ? la : lb; pa = tp; la = tl;
    }
    // from the PriorityQueue array (LDS words {priority bits, doc << 32}) with n nodes
    __device__ void load(const unsigned long long* hN, int n, int lane) {
        const int g0 = group0(lane), g1 = group1(lane);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int a = 4 * g0 + 1 + k, b = 4 * g1 + 1 + k;
            const unsigned long long va = a < n ? hN[a] : 0xFFFFFFFFull, vb = b < n ? hN[b] : 0xFFFFFFFFull;
            p0[k] = (uint32_t)va; l0[k] = ((uint32_t)k << 30) | ((uint32_t)(va >> 32) & RH_DOCM);
            p1[k] = (uint32_t)vb; l1[k] = ((uint32_t)k << 30) | ((uint32_t)(vb >> 32) & RH_DOCM);
        }
        cswap(p0[0], l0[0], p0[1], l0[1]); cswap(p0[2], l0[2], p0[3], l0[3]); cswap(p0[0], l0[0], p0[2], l0[2]); cswap(p0[1], l0[1], p0[3], l0[3]); cswap(p0[1], l0[1], p0[2], l0[2]);
        cswap(p1[0], l1[0], p1[1], l1[1]); cswap(p1[2], l1[2], p1[3], l1[3]); cswap(p1[0], l1[0], p1[2], l1[2]); cswap(p1[1], l1[1], p1[3], l1[3]); cswap(p1[1], l1[1], p1[2], l1[2]);
        const unsigned long long r = hN[0];
        rootP = (uint32_t)rfl_i((int)(uint32_t)r); rootD = (uint32_t)rfl_i((int)(uint32_t)(r >> 32));
        np0 = p0[0]; nl0 = l0[0]; np1 = p1[0]; nl1 = l1[0];
    }
    // The pending entry x replaces entry 0 — it keeps entry 0's sibling index: the node stays, its content changes — and takes its sorted place among
    // entries 1..3.  Branch-free and lane-local; an idle lane's x is its own entry 0 and nothing moves.  x > e  <=>  xp + (xl > el) > ep: sibling
    // indices of one group differ, so the comparison of the l words is the comparison of their top two bits (an idle sentinel entry wraps to 0: no move).
    __device__ __forceinline__ static void settle(uint32_t (&p)[4], uint32_t (&l)[4], uint32_t& np, uint32_t& nl) {
        const uint32_t xp = np, xl = (l[0] & RH_KM) | (nl & RH_DOCM);
        const bool c1 = xp + (xl > l[1] ? 1u : 0u) > p[1], c2 = xp + (xl > l[2] ? 1u : 0u) > p[2], c3 = xp + (xl > l[3] ? 1u : 0u) > p[3];
        const uint32_t a0 = c1 ? p[1] : xp, b0 = c1 ? l[1] : xl;
        const uint32_t a1 = c2 ? p[2] : (c1 ? xp : p[1]), b1 = c2 ? l[2] : (c1 ? xl : l[1]);
        const uint32_t a2 = c3 ? p[3] : (c2 ? xp : p[2]), b2 = c3 ? l[3] : (c2 ? xl : l[2]);
        const uint32_t a3 = c3 ? xp : p[3], b3 = c3 ? xl : l[3];
        p[0] = a0; l[0] = b0; p[1] = a1; l[1] = b1; p[2] = a2; l[2] = b2; p[3] = a3; l[3] = b3;
        np = a0; nl = b0;
    }
    // PriorityQueue.EnqueueDequeue for a priority above the root's (MoveDown from node 0, BCL rules: first minimal child, stop on <=)
    __device__ __forceinline__ static int child_group(int c, uint32_t ml) {              // 4 * c + 1 + sibling index, on the scalar unit (the compiler's own
        int r; const int k = rfl_i((int)(ml >> 30));                                        // choice is a VALU funnel shift and a v_readfirstlane back)
        asm("s_lshl2_add_u32 %0, %1, %2" : "=s"(r) : "s"(rfl_i(c)), "s"(k) : "scc");
        return r + 1;
    }
    __device__ __forceinline__ void replace_root(uint32_t np, uint32_t nd) {
        int hl = -1;                                                                        // the hole: entry 0 of lane hl (slot 0 unless in1); -1: none left to fill
        bool in1 = false;
        do {
            uint32_t mp = rdl_u(p0[0], 0);
            if (np <= mp) { rootP = np; rootD = nd; break; }
            uint32_t ml = rdl_u(l0[0], 0);
            rootP = mp; rootD = ml & RH_DOCM;
            hl = 0; int c = child_group(0, ml);                                            // c = the hole's node = its child group
            mp = rdl_u(p0[0], c); if (np <= mp) break;                                      // level 2: groups 1..4
            ml = rdl_u(l0[0], c); wrl2_u(np0, mp, nl0, ml, hl);
            hl = c; c = child_group(c, ml);
            mp = rdl_u(p0[0], c); if (np <= mp) break;                                      // level 3: groups 5..20
            ml = rdl_u(l0[0], c); wrl2_u(np0, mp, nl0, ml, hl);
            hl = c; c = child_group(c, ml);
            mp = rdl_u(p1[0], c - 21); if (np <= mp) break;                                 // level 4: groups 21..84 (slot 1)
            ml = rdl_u(l1[0], c - 21); wrl2_u(np0, mp, nl0, ml, hl);
            hl = c - 21; c = child_group(c, ml); in1 = true;                                // the hole is in slot 1 now
            if (c <= 127) {                                                                  // level 5: groups 85..127 (slot 0, lanes 21..63); its nodes have no children
                mp = rdl_u(p0[0], c - 64);
                if (np > mp) { ml = rdl_u(l0[0], c - 64); wrl2_u(np1, mp, nl1, ml, hl); hl = c - 64; in1 = false; }
            }
        } while (0);
        if (hl >= 0) { if (in1) wrl2_u(np1, np, nl1, nd, hl); else wrl2_u(np0, np, nl0, nd, hl); }
        settle(p0, l0, np0, nl0);
        settle(p1, l1, np1, nl1);
    }
    // back to PriorityQueue array order
    __device__ void store(infx_hit* __restrict__ out, int n, int lane) const {
        if (lane == 0) { infx_hit h; h.doc = (int32_t)rootD; h.score = __uint_as_float(rootP); out[0] = h; }
        const int g0 = group0(lane), g1 = group1(lane);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int a = 4 * g0 + 1 + (int)(l0[i] >> 30), b = 4 * g1 + 1 + (int)(l1[i] >> 30);
            if (a < n) { infx_hit h; h.doc = (int32_t)(l0[i] & RH_DOCM); h.score = __uint_as_float(p0[i]); out[a] = h; }
            if (b < n) { infx_hit h; h.doc = (int32_t)(l1[i] & RH_DOCM); h.score = __uint_as_float(p1[i]); out[b] = h; }
        }
    }
};

// UpdateTopK (:654-670) on one wave: WHeap while the heap fills, RHeap from the moment it is full (useReg: depth <= 512 and ids < 2^30)
struct TopKHeapW {
    WHeap H; RHeap R; bool inReg; int depth; uint32_t thetaBits; int useReg;
    __device__ __forceinline__ void init(unsigned long long* lds, int depth_, int useReg_) { H.rp = 0u; H.rd = 0; H.lds = lds; H.n = 0; inReg = false; depth = depth_; thetaBits = 0u; useReg = useReg_; R.np0 = R.nl0 = R.np1 = R.nl1 = 0u; R.rootP = 0u; R.rootD = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) { R.p0[i] = R.l0[i] = R.p1[i] = R.l1[i] = 0u; } }
    __device__ __forceinline__ bool full() const { return H.n >= depth; }
    __device__ __forceinline__ void offer(int32_t d, uint32_t sb) {          // d, sb wave-uniform
        if (H.n < depth) {
            // (round 5: an Enqueue that fetches the leaf's <= 5 ancestors with five lanes at once and moves the greater ones down in one parallel write
            //  was measured, too: 2.44 M against 2.26 M cycles per query — the sift-up rarely climbs more than a level, the lane set-up costs more)
            H.enqueue(d, sb);
            if (H.n == depth) {
                thetaBits = H.getp(0);
                if (useReg) { __builtin_amdgcn_wave_barrier(); R.load(H.lds, depth, (int)threadIdx.x); inReg = true; }
            }
        } else if (sb > thetaBits) {
            if (inReg) { R.replace_root(sb, (uint32_t)d); thetaBits = R.rootP; }
            else { H.enqueue_dequeue(d, sb); thetaBits = H.getp(0); }
        }
    }
    __device__ __forceinline__ void store(infx_hit* __restrict__ out, int lane) {
        if (inReg) { R.store(out, depth, lane); return; }
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < H.n; i += WAVE) { infx_hit h; const unsigned long long v = H.lds[i]; h.doc = (int32_t)(uint32_t)(v >> 32); h.score = __uint_as_float((uint32_t)v); out[i] = h; }
    }
};

// k_ex_heap: one wave per flagged query: UpdateTopK (:654-670) over the emitted candidates, chunk by chunk, on the wave-resident heap.
__global__ __launch_bounds__(WAVE) void k_ex_heap(Arena ar, const SelRule* __restrict__ rules, uint32_t* __restrict__ flagged, ExBufs xb,
                                                   infx_hit* __restrict__ out, uint32_t* __restrict__ outCount, int outStride, uint32_t* __restrict__ stats,
                                                   unsigned long long* __restrict__ prof, int useReg) {
    __shared__ unsigned long long hN[EXS_MAXDEPTH];
    long long pT0 = 0, pHeap = 0, pAll = 0; unsigned long long pRows = 0, pOps = 0;
    if (prof) pAll = (long long)__builtin_readcyclecounter();
    const int q = blockIdx.x, lane = threadIdx.x;
    if (flagged[q] != 1u) return;
    const int depth = rules[q].depth;
    const ExQuery Q = xb.queries[q];
    const unsigned long long qb = ar.qBase[q];
    TopKHeapW K; K.init(hN, depth, useReg);
    float theta = 0.f;                                       // stays 0 until the heap is full (:660-664)
    int bad = 0;
    // The chunk records are fetched 64 at a time (one per lane) and read out of the lanes with v_readlane; the first 64 emitted rows of the NEXT chunk
    // are requested before the current chunk is replayed.  Before, every chunk cost two dependent global round trips (record, then rows) on the one
    // wave that replays the query — ~300 chunks per query, the kernel's whole duration.
    for (uint32_t cb = 0; cb < Q.nChunks && !bad; cb += WAVE) {
        const uint32_t nb = min((uint32_t)WAVE, Q.nChunks - cb);
        ExChunk mine; mine.q = 0; mine.i0 = 0; mine.n = 0; mine.full = 0; mine.theta = 0.f; mine.lo = 0.f; mine.hi = 0.f; mine.cnt = 0;
        if ((uint32_t)lane < nb) mine = xb.chunks[Q.chunk0 + cb + lane];
        infx_hit pre; pre.doc = 0; pre.score = 0.f;
        { const uint32_t i00 = rdl_u(mine.i0, 0), cnt0 = rdl_u(mine.cnt, 0); if ((uint32_t)lane < cnt0) pre = (xb.out + qb + i00)[lane]; }
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t i0 = rdl_u(mine.i0, (int)j), cnt = rdl_u(mine.cnt, (int)j), full = rdl_u(mine.full, (int)j);
            const float lo = rdl_f(mine.lo, (int)j), hi = rdl_f(mine.hi, (int)j);
            infx_hit h = pre;
            if (j + 1 < nb) {
                const uint32_t i0n = rdl_u(mine.i0, (int)j + 1), cntn = rdl_u(mine.cnt, (int)j + 1);
                pre.doc = 0; pre.score = 0.f;
                if ((uint32_t)lane < cntn) pre = (xb.out + qb + i0n)[lane];
            }
            // the chunk's skip decisions were taken against the predicted threshold: they are the reference's iff the exact threshold at the
            // chunk start lies in [lo, hi); the "heap full" prediction must hold as well
            if (!(lo <= theta && theta < hi) || (full != 0u) != K.full()) { bad = 1; break; }
            const infx_hit* R = xb.out + qb + i0;
            for (uint32_t b0 = 0; b0 < cnt; b0 += WAVE) {
                if (b0) { h.doc = 0; h.score = 0.f; if (b0 + lane < cnt) h = R[b0 + lane]; }
                unsigned long long w = __ballot(b0 + lane < cnt && (!K.full() || h.score > theta));
                if (prof) { pRows += min((uint32_t)WAVE, cnt - b0); pOps += (unsigned long long)__popcll(w); pT0 = (long long)__builtin_readcyclecounter(); }
                while (w) {
                    const int b = __ffsll((long long)w) - 1; w &= w - 1;
                    const uint32_t sb = rdl_u(__float_as_uint(h.score), b); const int32_t d = __builtin_amdgcn_readlane(h.doc, b);
                    K.offer(d, sb);
                }
                theta = __uint_as_float(K.thetaBits);
                if (prof) pHeap += (long long)__builtin_readcyclecounter() - pT0;
            }
        }
    }
    if (prof && lane == 0) { unsigned long long* P = prof + (size_t)q * EXP_WORDS; P[0] = (unsigned long long)((long long)__builtin_readcyclecounter() - pAll); P[1] = (unsigned long long)pHeap; P[2] = pRows; P[3] = pOps; P[4] = Q.nChunks; }
    if (bad) { if (lane == 0) { flagged[q] = 2u; if (stats) atomicAdd(&stats[2], 1u); } return; }      // k_exact1 replays this query
    K.store(out + (size_t)q * outStride, lane);
    if (lane == 0) { outCount[q] = (uint32_t)K.H.n; flagged[q] = 0u; if (stats) atomicAdd(&stats[0], 1u); }
}
