// k_exact1 — exact replay of the reference's Stage-1 order effects for queries whose top-`depth` cut is ambiguous.
//
// Two things make Bm25Scorer.Search's result depend on the ORDER in which it processes candidates, not only on their postings:
//   Q9   ScoreBlockStruct (Indexing/Bm25Scorer.cs:332-445) scores the matches of a (<= 4096-candidate chunk, term) pair in groups of eight
//        with the Vector256 formula  K1 * ((1-B) + (B/avgdl) * dl)  and the  mc % 8  trailing matches with ComputeTermScore
//        (:643-652),  K1 * (1 - B + B * (dl / avgdl))  — the two round differently for ~10 % of the (tf, dl) pairs, so a candidate's
//        fp32 score depends on its POSITION among the chunk's matches of every term, and on the MaxScore skip
//        (cur + maxScore + suffix <= threshold, :350-368) that removes candidates from the match list;
//   Q10  UpdateTopK (:654-670) keeps the top-`depth` in a BCL PriorityQueue<int,float> (4-ary min-heap): an arriving score equal to the
//        threshold is rejected, and WHICH of several minimum-score entries a better arrival evicts is decided by the heap layout.
// k_accumulate scores every posting with the Vector256 formula and k_select cuts by (score, doc id): identical to the reference unless
// rows near the cut have scores within a few ulp of each other — structural ties are common (same matched terms, same document length).
// k_select flags such queries.  The production path is the parallel replay of exact3.hip.inc (k_ex_walk / k_ex_theta / k_ex_chunk / k_ex_heap); this
// kernel is the literal form — one workgroup re-runs the reference's sequential algorithm for a query, parallelised only inside a
// (chunk, term) step — kept as the fallback for queries the parallel form cannot certify, and as its cross-check (INFX_EXACT_SLOW=1):
//   candidates   = the query's arena rows that pass its tier rule, in ascending doc id through the (query, range) directory;
//   containers   = 65 536-id Roaring containers, chunks of <= 4096 candidates inside one (ProcessBlockedCandidates :195-280);
//   per term     = match list from the rows' hit masks (2 bits per term: absent / tf 1 / tf 2 / other -> posting lookup) minus the
//                  MaxScore-skipped candidates; block scan -> position of every match -> formula choice -> score update;
//   per chunk    = UpdateTopK in doc order on an LDS 4-ary heap with the BCL's sift rules (oracle/dotnet.hpp restates the same).
// The result (exact set, exact fp32 scores) replaces the query's k_select rows.  Follows oracle-side restatement order exactly:
// Bm25Scorer.cs:56-193 (Search), :282-330 (ProcessChunk), :524-533 (suffix sums), :447-461 (PopulateResultHeapFromPruning).
#define EX_THREADS 256
#define EX_CHUNK 4096

struct DevRefTerm { float idf, maxScore; int32_t termId; uint32_t unit; };   // one per query term, Bm25Scorer order; unit: virtual term (tf == 1)

struct ExHeap {            // PriorityQueue<int,float>: array-backed 4-ary min-heap (nodes = (doc, score))
    int32_t* d; float* p; int n;
    __device__ void move_up(int32_t nd, float np, int idx) {
        while (idx > 0) { const int parent = (idx - 1) >> 2; if (np < p[parent]) { d[idx] = d[parent]; p[idx] = p[parent]; idx = parent; } else break; }
        d[idx] = nd; p[idx] = np;
    }
    __device__ void move_down(int32_t nd, float np, int idx) {
        int i;
        while ((i = (idx << 2) + 1) < n) {
            // the four children are read as independent LDS loads (one latency per level); first minimal child wins, as in the BCL loop
            const float c0 = p[i], c1 = i + 1 < n ? p[i + 1] : __builtin_inff(), c2 = i + 2 < n ? p[i + 2] : __builtin_inff(), c3 = i + 3 < n ? p[i + 3] : __builtin_inff();
            float mp = c0; int mi = i;
            if (c1 < mp) { mp = c1; mi = i + 1; }
            if (c2 < mp) { mp = c2; mi = i + 2; }
            if (c3 < mp) { mp = c3; mi = i + 3; }
            if (np <= mp) break;
            d[idx] = d[mi]; p[idx] = mp; idx = mi;
        }
        d[idx] = nd; p[idx] = np;
    }
    __device__ void enqueue(int32_t nd, float np) { n++; move_up(nd, np, n - 1); }
    __device__ void enqueue_dequeue(int32_t nd, float np) { if (n > 0 && np > p[0]) move_down(nd, np, 0); }
};

// exclusive block scan of one value per thread (EX_THREADS = 4 waves); part: 2 x 5 uint32 in LDS, tog alternates the buffer so that one
// barrier per scan suffices
__device__ __forceinline__ uint32_t ex_scan(uint32_t v, uint32_t* part, int& tog, int tid, uint32_t& total) {
    const int lane = tid & 63, w = tid >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if (lane >= d) incl += x; }
    uint32_t* P = part + tog * 4; tog ^= 1;
    if (lane == WAVE - 1) P[w] = incl;
    __syncthreads();
    const uint32_t p0 = P[0], p1 = P[1], p2 = P[2], p3 = P[3];
    total = p0 + p1 + p2 + p3;
    const uint32_t before = (w > 0 ? p0 : 0u) + (w > 1 ? p1 : 0u) + (w > 2 ? p2 : 0u);
    return before + incl - v;
}

__device__ __forceinline__ float ex_tf_lookup(const DevIndex& ix, int32_t termId, int32_t localDoc) {
    uint64_t lo = ix.postOff[termId], hi = ix.postOff[termId + 1];
    const uint64_t p = lower_bound_post(ix.postDoc, lo, hi, localDoc, ix.packed);
    if (p >= hi || post_doc(ix.postDoc[p], ix.packed) != localDoc) return 1.0f;        // cannot happen: the row's mask says the posting exists
    return ix.packed ? (float)((uint32_t)ix.postDoc[p] & 0xFFu) : (float)ix.postW[p];
}

__global__ __launch_bounds__(EX_THREADS) void k_exact1(DevIndex ix, const DevQuery* __restrict__ queries, const DevRefTerm* __restrict__ refTerms, Arena ar,
                                                        const SelRule* __restrict__ rules, const uint32_t* __restrict__ flagged, uint32_t want, float avgdlIn,
                                                        infx_hit* __restrict__ out, uint32_t* __restrict__ outCount, int outStride, int depthCap, uint32_t* __restrict__ stats,
                                                        uint32_t* __restrict__ chainState, const uint32_t* __restrict__ chainNeed) {
    // chainState != nullptr (document shards, the sequential fallback): the heap is CONTINUED — per query 2 + 2 * depthCap words {n, threshold bits,
    // doc[depthCap], score bits[depthCap]} in PriorityQueue array order, as the shard before this one left it — over this shard's candidates and
    // written back; the last shard's state is the reference's final heap.  Entries carry global internal ids.
    const int q = blockIdx.x, tid = threadIdx.x;
    if (chainState ? chainNeed[q] == 0u : flagged[q] != want) return;
    const int MW = ar.maskWords;
    // Masks of up to two words per row (<= 64 reference terms: every ordinary batch) are staged in LDS; a batch that holds a query of 65 .. 128 terms keeps four words
    // per row, which do not fit beside the chunk (139 KB): the chunk then keeps the ROW index and reads the masks from the arena (round 6: the exact cut for such
    // queries — they are replayed by this kernel only).
    const int MWL = MW <= 2 ? MW : 1;                                             // words per slot in LDS (MW > 2: one u64 slot holding the arena row index)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* sMask = (unsigned long long*)smem;                        // (EX_CHUNK + EX_THREADS) * MWL
    int32_t* sDoc = (int32_t*)(sMask + (size_t)(EX_CHUNK + EX_THREADS) * MWL);     // EX_CHUNK + EX_THREADS (tail = spill of the tile that crossed the chunk end)
    float* sCur = (float*)(sDoc + EX_CHUNK + EX_THREADS);                         // EX_CHUNK
    int32_t* hD = (int32_t*)(sCur + EX_CHUNK);                                     // depthCap
    float* hP = (float*)(hD + depthCap);                                          // depthCap
    float* sSuf = hP + depthCap;                                                  // INFX_MAX_QUERY_TERMS + 1
    uint32_t* sPre = (uint32_t*)(sSuf + INFX_MAX_QUERY_TERMS + 1);                // 130: row prefix over the container's ranges
    uint32_t* sDirOff = sPre + 130;                                               // 129
    uint32_t* sPart = sDirOff + 129;                                              // 8
    uint16_t* sList = (uint16_t*)(sPart + 8);                                     // EX_CHUNK
    __shared__ int shHeapN; __shared__ float shTheta;

    const DevQuery Q = queries[q];
    const SelRule rule = rules[q];
    const int depth = rule.depth;
    const int nRef = (int)Q.numRef;
    const DevRefTerm* RT = refTerms + Q.refOff;
    const unsigned long long qb = ar.qBase[q];
    const uint2* dir = ar.dir + (unsigned long long)q * ix.nRanges;
    const float avgdl = avgdlIn > 0.f ? avgdlIn : 1.f;
    int tog = 0;
    auto mask_word = [&](int j, int wsel) -> unsigned long long { return MW <= 2 ? sMask[(size_t)j * MW + wsel] : ar.mask[sMask[j] * (unsigned long long)MW + wsel]; };
    uint32_t* const cst = chainState ? chainState + (size_t)q * (2 + 2 * (size_t)depthCap) : nullptr;
    if (cst) { const int n0 = (int)cst[0]; for (int i = tid; i < n0; i += EX_THREADS) { hD[i] = (int32_t)cst[2 + i]; hP[i] = __uint_as_float(cst[2 + depthCap + i]); } }
    if (tid == 0) {
        shHeapN = cst ? (int)cst[0] : 0; shTheta = cst ? __uint_as_float(cst[1]) : 0.f;
        sSuf[nRef] = 0.f;
        for (int i = nRef - 1; i >= 0; i--) sSuf[i] = sSuf[i + 1] + RT[i].maxScore;       // ComputeSuffixSums :524-533
    }
    __syncthreads();
    ExHeap H; H.d = hD; H.p = hP; H.n = shHeapN;     // only thread 0's copy is live

    // ---- one chunk: the terms in Bm25Scorer order, then UpdateTopK in doc order -----------------------------------------------
    auto process_chunk = [&](const int n) {
        const int per = (n + EX_THREADS - 1) / EX_THREADS;
        const int j0 = min(n, tid * per), j1 = min(n, j0 + per);
        for (int j = j0; j < j1; j++) sCur[j] = 0.f;
        const float th = shTheta;
        for (int t = 0; t < nRef; t++) {
            const DevRefTerm rt = RT[t];
            if (!(rt.idf > 0.f)) continue;                                        // :301-309
            const float ms = rt.maxScore, rem = sSuf[t + 1];
            const int wsel = t >> 5, sh = (t & 31) * 2;
            uint32_t cnt = 0;
            for (int j = j0; j < j1; j++) {
                const uint32_t code = (uint32_t)(mask_word(j, wsel) >> sh) & 3u;
                if (code && !((sCur[j] + ms) + rem <= th)) cnt++;                 // :350-368 (topK < int.MaxValue always)
            }
            uint32_t mc; uint32_t i = ex_scan(cnt, sPart, tog, tid, mc);
            if (mc == 0) continue;
            const uint32_t lim = mc & ~7u;                                        // Vector256 groups of eight, scalar tail (:395-444)
            for (int j = j0; j < j1; j++) {
                const uint32_t code = (uint32_t)(mask_word(j, wsel) >> sh) & 3u;
                const float cur = sCur[j];
                if (!code || ((cur + ms) + rem <= th)) continue;
                const int32_t dl_doc = sDoc[j];
                const float tf = (rt.unit || code == 1u) ? 1.0f : (code == 2u ? 2.0f : ex_tf_lookup(ix, rt.termId, dl_doc));
                float sc;
                if (i < lim) {
                    const float denom = tf + ix.docNorm[dl_doc];                  // docNorm = K1 * ((1-B) + (B/avgdl) * dl), the lane formula
                    const float core = (tf * (1.2f + 1.0f)) / denom;
                    sc = rt.idf * (core + 1.0f);
                } else {                                                          // ComputeTermScore :643-652
                    float dl = ix.docLen[dl_doc]; if (dl <= 0.f) dl = 1.f;
                    const float normFactor = 1.2f * (1.f - 0.75f + 0.75f * (dl / avgdl));
                    const float denom = tf + normFactor;
                    if (denom <= 0.f) sc = 0.f;
                    else { const float core = (tf * (1.2f + 1.f)) / denom; sc = rt.idf * (core + 1.0f); }
                }
                sCur[j] = cur + sc;
                i++;
            }
        }
        // flush (:316-329): positive scores to UpdateTopK in chunk order; a score <= the chunk-start threshold cannot enter a full heap
        const bool full = shHeapN >= depth;
        uint32_t cp = 0;
        // a deleted document (Bm25Scorer.cs:322-323) keeps its place in the chunk but is never offered to UpdateTopK
        const uint8_t* qdel = q_deleted(ix, (uint32_t)q);
        const uint8_t* del = qdel ? qdel + ix.docBase : nullptr;
        for (int j = j0; j < j1; j++) { const float s = sCur[j]; if (s > 0.f && (!full || s > th) && !(del && del[sDoc[j]])) cp++; }
        uint32_t np; uint32_t o = ex_scan(cp, sPart, tog, tid, np);
        for (int j = j0; j < j1; j++) { const float s = sCur[j]; if (s > 0.f && (!full || s > th) && !(del && del[sDoc[j]])) sList[o++] = (uint16_t)j; }
        __syncthreads();
        if (tid == 0) {
            float theta = shTheta;
            for (uint32_t x = 0; x < np; x++) {
                const int j = sList[x]; const float s = sCur[j]; const int32_t d = sDoc[j] + ix.docBase;     // heap entries carry global ids
                if (H.n < depth) { H.enqueue(d, s); if (H.n == depth) theta = H.p[0]; }
                else if (s > theta) { H.enqueue_dequeue(d, s); theta = H.p[0]; }
            }
            shTheta = theta; shHeapN = H.n;
        }
        __syncthreads();
    };

    const int rpc = 65536 / ix.R;                                                 // ranges per Roaring container (R <= 16384)
    const int nCont = (ix.nRanges + rpc - 1) / rpc;
    int fill = 0;
    for (int c = 0; c < nCont; c++) {
        const int r0 = c * rpc, nr = min(ix.nRanges, r0 + rpc) - r0;
        if (tid < nr) { const uint2 e = dir[r0 + tid]; sPre[tid + 1] = e.y; sDirOff[tid] = e.x; }
        __syncthreads();
        if (tid == 0) { uint32_t run = 0; sPre[0] = 0; for (int k = 1; k <= nr; k++) { run += sPre[k]; sPre[k] = run; } }
        __syncthreads();
        const uint32_t total = sPre[nr];
        for (uint32_t v0 = 0; v0 < total; v0 += EX_THREADS) {
            const uint32_t v = v0 + tid; bool pass = false; unsigned long long row = 0;
            if (v < total) {
                int lo = 0, hi = nr;                                              // last k with sPre[k] <= v
                while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (sPre[m] <= v) lo = m; else hi = m; }
                row = qb + sDirOff[lo] + (v - sPre[lo]);
                pass = sel_pass(rule, ar.cls[row]);
            }
            uint32_t tileCnt; const uint32_t pos = ex_scan(pass ? 1u : 0u, sPart, tog, tid, tileCnt);
            if (pass) {
                const int slot = fill + (int)pos;                                 // < EX_CHUNK + EX_THREADS
                sDoc[slot] = ar.doc[row] - ix.docBase;
                if (MW <= 2) { for (int w = 0; w < MW; w++) sMask[(size_t)slot * MW + w] = ar.mask[row * (unsigned long long)MW + w]; }
                else sMask[slot] = row;
            }
            __syncthreads();
            const int nf = fill + (int)tileCnt;
            if (nf >= EX_CHUNK) {
                process_chunk(EX_CHUNK);
                const int restN = nf - EX_CHUNK;                                  // < EX_THREADS
                int32_t dd = 0; unsigned long long m0 = 0, m1 = 0;
                if (tid < restN) { dd = sDoc[EX_CHUNK + tid]; m0 = sMask[(size_t)(EX_CHUNK + tid) * MWL]; if (MWL > 1) m1 = sMask[(size_t)(EX_CHUNK + tid) * MWL + 1]; }
                __syncthreads();
                if (tid < restN) { sDoc[tid] = dd; sMask[(size_t)tid * MWL] = m0; if (MWL > 1) sMask[(size_t)tid * MWL + 1] = m1; }
                __syncthreads();
                fill = restN;
            } else fill = nf;
        }
        if (fill > 0) { process_chunk(fill); fill = 0; }
        __syncthreads();
    }
    // PopulateResultHeapFromPruning: every heap entry reaches the result heap (<= depth of them); k_prep2 re-sorts into ConsolidateSegments order
    const int hn = shHeapN;
    if (cst) {
        for (int i = tid; i < hn; i += EX_THREADS) { cst[2 + i] = (uint32_t)hD[i]; cst[2 + depthCap + i] = __float_as_uint(hP[i]); }
        if (tid == 0) { cst[0] = (uint32_t)hn; cst[1] = __float_as_uint(shTheta); if (stats) atomicAdd(&stats[1], 1u); }
        return;
    }
    for (int i = tid; i < hn; i += EX_THREADS) { infx_hit h; h.doc = hD[i]; h.score = hP[i]; out[(size_t)q * outStride + i] = h; }
    if (tid == 0) { outCount[q] = (uint32_t)hn; if (stats) atomicAdd(&stats[want == 2u ? 1 : 0], 1u); }
}


