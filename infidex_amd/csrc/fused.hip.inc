// Device-resident batch pipeline behind infx_search_fused (unsharded index): after k_accumulate the tier rules, the top-`depth`
// selection, the coverage-stage candidate assembly, the Stage-2 scoring and the final ordering / truncation all run on the GPU,
// back to back on one stream; only the final max_results rows per query return to the host.  Included by infidex_hip.hip.
//
//   k_rules     TieredCandidateSelector tier decision from the class histogram          (TieredCandidateSelector.cs:128-322)
//   k_prep2     SearchPipeline.ExecuteCoverageStage candidate assembly                   (SearchPipeline.cs:330-420):
//               Stage-1 list in ConsolidateSegments order, WordMatcher overlap / first-unique ids, docIndex 0/1, candidate rows
//   k_finalize  TopKHeap + ConsolidateSegments + CalculateTruncationIndex                (SearchPipeline.cs:422-560, ResultProcessor)

#define P2_THREADS 256
#define P2_CAP 2048          // ids gathered per WordMatcher merge round
#define P2_MAXLISTS 256
#define FQ_SKIP 1u           // blank / unsupported query: no results
#define FQ_SHORT 2u          // 1..3 characters, no delimiter (SearchPipeline.cs:108-120)
#define FQ_SHORTSKIP 4u      // short query whose prefix population exceeds 500: coverage skipped
#define FQ_COV 8u            // coverage enabled for this query
#define FQ_UNSUPPORTED 16u   // reported as flag bit0 in the result

struct FusedMeta { uint32_t s1Count, candCount; int32_t idx0, idx1; uint32_t runCov, wmAny, pad0, pad1; };

__global__ void k_rules(const infx_query* __restrict__ qs, const uint32_t* __restrict__ counts, SelRule* __restrict__ rules, uint32_t nq) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    rules[i] = make_rule(qs[i], counts + (size_t)i * INFX_NCLASS);
}

// ---- workgroup helpers ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wg_bitonic_i32(int32_t* a, uint32_t n2, int tid, int nth) {     // ascending; pad with INT_MAX
    for (uint32_t k = 2; k <= n2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < n2; i += nth) {
                uint32_t ixj = i ^ j;
                if (ixj > i) { int32_t x = a[i], y = a[ixj]; bool up = (i & k) == 0; if (up ? (x > y) : (x < y)) { a[i] = y; a[ixj] = x; } }
            }
            __syncthreads();
        }
}
template <class Less> __device__ __forceinline__ void wg_bitonic_idx(uint16_t* idx, uint32_t n2, int tid, int nth, Less less) {   // ascending by `less`
    for (uint32_t k = 2; k <= n2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < n2; i += nth) {
                uint32_t ixj = i ^ j;
                if (ixj > i) { uint16_t x = idx[i], y = idx[ixj]; bool up = (i & k) == 0; if (up ? less(y, x) : less(x, y)) { idx[i] = y; idx[ixj] = x; } }
            }
            __syncthreads();
        }
}
// exclusive scan of flag[0..n) (0/1 bytes) into pos[0..n); returns the total.  part: >= nth uint32 of scratch.
__device__ __forceinline__ uint32_t wg_scan_flags(const uint8_t* flag, uint32_t* pos, uint32_t n, uint32_t* part, int tid, int nth) {
    const uint32_t per = (n + nth - 1) / nth, b0 = min(n, (uint32_t)tid * per), b1 = min(n, b0 + per);
    uint32_t s = 0; for (uint32_t i = b0; i < b1; i++) s += flag[i];
    part[tid] = s; __syncthreads();
    if (tid == 0) { uint32_t run = 0; for (int i = 0; i < nth; i++) { uint32_t x = part[i]; part[i] = run; run += x; } part[nth] = run; }
    __syncthreads();
    uint32_t run = part[tid];
    for (uint32_t i = b0; i < b1; i++) { pos[i] = run; run += flag[i]; }
    const uint32_t total = part[nth];
    __syncthreads();
    return total;
}
__device__ __forceinline__ bool sorted_contains(const int32_t* a, uint32_t n, int32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { uint32_t m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
    return lo < n && a[lo] == v;
}

#ifdef SEL_PROF
__device__ unsigned long long* g_p2Prof = nullptr;
#define P2P(i) do { if (g_p2Prof && tid == 0) g_p2Prof[(size_t)qi * 8 + (i)] = wall_clock64(); } while (0)
#else
#define P2P(i)
#endif
// ---- k_prep2: one workgroup per query ---------------------------------------------------------------------------------------
// dynamic LDS layout (Dp = power of two >= depth):
//   sScore[Dp] f32 | sDoc[Dp] i32 | sTop[Dp] i32 | sUniq[Dp] i32 | sPos[max(Dp, P2_CAP)] u32 | sBuf[P2_CAP] i32 | sKey[Dp] i64 |
//   sIdx[Dp] u16 | sFlag[max(Dp, P2_CAP)] u8 | per-list: lBase[256] u64, lLen[256] u32, lPos[256] u32, lCnt[256] u32 | part[257] u32
__global__ __launch_bounds__(P2_THREADS) void k_prep2(DevIndex ix, const infx_hit* __restrict__ hits, const uint32_t* __restrict__ hitCount, int hitStride,
                                                       int W, int nd, int Dall,
                                                       const infx_fused_query* __restrict__ fqs, const infx_wm_list* __restrict__ lists,
                                                       const int32_t* __restrict__ owned, int depth, int Dp,
                                                       infx_hit* __restrict__ s1Out, infx_cov_cand* __restrict__ cands, int32_t* __restrict__ pairs, FusedMeta* __restrict__ metas) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t Pp = (uint32_t)max(Dp, P2_CAP);
    float* sScore = (float*)smem;
    int32_t* sDoc = (int32_t*)(sScore + Dp);
    int32_t* sTop = sDoc + Dp;
    int32_t* sUniq = sTop + Dp;
    uint32_t* sPos = (uint32_t*)(sUniq + Dp);
    int32_t* sBuf = (int32_t*)(sPos + Pp);
    long long* sKey = (long long*)(sBuf + P2_CAP);
    uint16_t* sIdx = (uint16_t*)(sKey + Dp);
    uint8_t* sFlag = (uint8_t*)(sIdx + Dp);
    unsigned long long* lBase = (unsigned long long*)(sFlag + Pp);
    uint32_t* lLen = (uint32_t*)(lBase + P2_MAXLISTS);
    uint32_t* lPos = lLen + P2_MAXLISTS;
    uint32_t* lCnt = lPos + P2_MAXLISTS;
    uint32_t* part = lCnt + P2_MAXLISTS;        // P2_THREADS + 1
    unsigned long long* sMerge = (unsigned long long*)(part + P2_THREADS + 2);   // Dall, only when W > 1 (8-byte aligned: all sizes above are)
    __shared__ uint32_t shA, shB; __shared__ int32_t shT, shL0, shL1;

    const int qi = blockIdx.x, tid = threadIdx.x;
    const infx_fused_query FQ = fqs[qi];
    const uint32_t stride = 2u * (uint32_t)depth;
    infx_cov_cand* myC = cands + (size_t)qi * stride;
    FusedMeta M; M.s1Count = 0; M.candCount = 0; M.idx0 = -1; M.idx1 = -1; M.runCov = 0; M.wmAny = 0; M.pad0 = 0; M.pad1 = 0;
    int32_t* myP = pairs + (size_t)qi * stride;
    P2P(0);
    for (uint32_t i = tid; i < stride; i += P2_THREADS) { infx_cov_cand c; c.query = 0xFFFFFFFFu; c.doc = -1; c.base_score = 0.f; c.want_lcs = 0; myC[i] = c; myP[i] = -1; }
    if (FQ.flags & FQ_SKIP) { if (tid == 0) metas[qi] = M; return; }

    // ---- Stage-1 list in ConsolidateSegments order: score descending, DocumentKey ascending -------------------------------
    uint32_t c = 0;
    if (W <= 1) {
        c = FQ.dev >= 0 ? min(hitCount[FQ.dev], (uint32_t)depth) : 0u;
        for (uint32_t i = tid; i < c; i += P2_THREADS) { infx_hit h = hits[(size_t)FQ.dev * hitStride + i]; sScore[i] = h.score; sDoc[i] = h.doc; }
    } else if (FQ.dev >= 0) {
        // global top-`depth` = best `depth` of the union of the per-shard top-`depth` lists, in k_select's order (score desc, doc asc)
        uint32_t tot = 0;
        for (int w = 0; w < W; w++) {
            const uint32_t cw = min(hitCount[(size_t)w * nd + FQ.dev], (uint32_t)depth);
            const infx_hit* H = hits + ((size_t)w * nd + FQ.dev) * hitStride;
            for (uint32_t i = tid; i < cw; i += P2_THREADS) { const infx_hit h = H[i]; sMerge[tot + i] = ((unsigned long long)__float_as_uint(h.score) << 32) | (0xFFFFFFFFu - (uint32_t)h.doc); }
            tot += cw;
        }
        uint32_t m2 = 2; while (m2 < tot) m2 <<= 1;
        for (uint32_t i = tot + tid; i < m2; i += P2_THREADS) sMerge[i] = 0ull;
        __syncthreads();
        for (uint32_t k = 2; k <= m2; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < m2; i += P2_THREADS) {
                    uint32_t ixj = i ^ j;
                    if (ixj > i) { unsigned long long a = sMerge[i], b = sMerge[ixj]; bool up = (i & k) == 0; if (up ? (a < b) : (a > b)) { sMerge[i] = b; sMerge[ixj] = a; } }
                }
                __syncthreads();
            }
        c = min(tot, (uint32_t)depth);
        for (uint32_t i = tid; i < c; i += P2_THREADS) { const unsigned long long k = sMerge[i]; sDoc[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)k); sScore[i] = __uint_as_float((uint32_t)(k >> 32)); }
    }
    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)Dp; i += P2_THREADS) {
        if (i < c) sKey[i] = ix.docKeyAll[sDoc[i]];
        else { sScore[i] = -1.f; sDoc[i] = 0x7FFFFFFF; sKey[i] = 0x7FFFFFFFFFFFFFFFll; }
        sIdx[i] = (uint16_t)i;
    }
    __syncthreads();
    uint32_t c2 = 2; while (c2 < c) c2 <<= 1;
    if (c > 1) wg_bitonic_idx(sIdx, c2, tid, P2_THREADS, [&](uint16_t a, uint16_t b) {
        if (sScore[a] != sScore[b]) return sScore[a] > sScore[b];
        return sKey[a] < sKey[b]; });
    // permute into sorted order through sTop/sUniq/sPos as scratch
    for (uint32_t i = tid; i < c; i += P2_THREADS) { uint16_t s = sIdx[i]; sTop[i] = sDoc[s]; sUniq[i] = __float_as_int(sScore[s]); }
    __syncthreads();
    for (uint32_t i = tid; i < c; i += P2_THREADS) { sDoc[i] = sTop[i]; sScore[i] = __int_as_float(sUniq[i]); }
    __syncthreads();
    for (uint32_t i = tid; i < c; i += P2_THREADS) { infx_hit h; h.doc = sDoc[i]; h.score = sScore[i]; s1Out[(size_t)qi * depth + i] = h; }
    M.s1Count = c;
    P2P(1);

    const bool isShort = (FQ.flags & FQ_SHORT) != 0;
    if ((isShort && (int)c >= FQ.max_results) || !(FQ.flags & FQ_COV) || (FQ.flags & FQ_SHORTSKIP)) { if (tid == 0) metas[qi] = M; return; }
    M.runCov = 1;

    // ---- WordMatcher lists ---------------------------------------------------------------------------------------------------
    const uint32_t nL = min(FQ.wm_count, (uint32_t)P2_MAXLISTS);
    for (uint32_t l = tid; l < nL; l += P2_THREADS) {
        const infx_wm_list L = lists[FQ.wm_off + l];
        const int32_t* p = L.src == 0 ? ix.wmExact : (L.src == 1 ? ix.wmLd1 : owned);
        lBase[l] = (unsigned long long)(uintptr_t)(p + L.off); lLen[l] = L.len; lPos[l] = 0;
    }
    M.wmAny = nL > 0 ? 1u : 0u;
    // sortedTop
    const uint32_t ntop = c;
    for (uint32_t i = tid; i < (uint32_t)Dp; i += P2_THREADS) sTop[i] = i < ntop ? sDoc[i] : 0x7FFFFFFF;
    __syncthreads();
    uint32_t t2 = 2; while (t2 < ntop) t2 <<= 1;
    if (ntop > 1) wg_bitonic_i32(sTop, t2, tid, P2_THREADS);
    P2P(2);
#ifdef SEL_PROF
    if (g_p2Prof && tid == 0) g_p2Prof[(size_t)qi * 8 + 6] = nL;
#endif
    // overlap = sortedTop ids present in any list (ascending)
    for (uint32_t i = tid; i < ntop; i += P2_THREADS) {
        const int32_t d = sTop[i]; uint8_t f = 0;
        for (uint32_t l = 0; l < nL && !f; l++) f = sorted_contains((const int32_t*)(uintptr_t)lBase[l], lLen[l], d) ? 1 : 0;
        sFlag[i] = f;
    }
    __syncthreads();
    const uint32_t nOv = wg_scan_flags(sFlag, sPos, ntop, part, tid, P2_THREADS);
    for (uint32_t i = tid; i < ntop; i += P2_THREADS) if (sFlag[i]) { infx_cov_cand cc; cc.query = (uint32_t)qi; cc.doc = sTop[i]; cc.base_score = 0.f; cc.want_lcs = 0; myC[sPos[i]] = cc; }
    const uint32_t wmLimit = (uint32_t)max(0, depth - (int)nOv);
    const uint32_t need = max(wmLimit, 2u);
    __syncthreads();
    P2P(3);

    // ---- first `need` ids of the union of the lists, ascending, that are not in sortedTop (WordMatcher-only candidates) ----
    // Rounds: T = the smallest "window end" value over the lists (a window = the next B unread ids of a list); every unread id
    // <= T lies inside its list's window, so one round gathers at most nL * B <= P2_CAP ids, sorts and de-duplicates them.
    // Deleted documents (SearchPipeline.cs:463-465, 532-537): a deleted WordMatcher-only id still counts against wmLimit but is not scored and
    // gets no docIndex — lv0/lv1 track the first two LIVE WordMatcher-only ids (only needed while Stage 1 supplies fewer than two documents).
    const uint8_t* del = q_deleted(ix, (uint32_t)nd + (uint32_t)qi);      // (the table holds the Stage-1 queries' entries, then the fused queries')
    int32_t lv0 = -1, lv1 = -1;
    uint32_t nu = 0;
    while ((nu < need || (del && ntop + (lv0 >= 0) + (lv1 >= 0) < 2u)) && nL > 0) {
        if (tid == 0) { shA = 0; shT = 0x7FFFFFFF; shL0 = 0x7FFFFFFF; shL1 = 0x7FFFFFFF; }
        __syncthreads();
        if ((uint32_t)tid < nL && lPos[tid] < lLen[tid]) atomicAdd(&shA, 1u);
        __syncthreads();
        const uint32_t nAct = shA;
        if (nAct == 0) break;
        const uint32_t B = max(1u, (uint32_t)P2_CAP / nAct);
        if ((uint32_t)tid < nL && lPos[tid] < lLen[tid]) {
            const int32_t* p = (const int32_t*)(uintptr_t)lBase[tid];
            const uint32_t e = min(lPos[tid] + B, lLen[tid]);
            atomicMin(&shT, p[e - 1]);
        }
        __syncthreads();
        const int32_t T = shT;
        if ((uint32_t)tid < nL) {
            uint32_t cnt = 0;
            if (lPos[tid] < lLen[tid]) {
                const int32_t* p = (const int32_t*)(uintptr_t)lBase[tid];
                uint32_t lo = lPos[tid], hi = min(lPos[tid] + B, lLen[tid]);
                while (lo < hi) { uint32_t m = (lo + hi) >> 1; if (p[m] <= T) lo = m + 1; else hi = m; }
                cnt = lo - lPos[tid];
            }
            lCnt[tid] = cnt;
        }
        __syncthreads();
        if (tid == 0) { uint32_t run = 0; for (uint32_t l = 0; l < nL; l++) { uint32_t x = lCnt[l]; part[l] = run; run += x; } shB = run; }
        __syncthreads();
        const uint32_t tot = shB;
        for (uint32_t l = 0; l < nL; l++) {
            const uint32_t cnt = lCnt[l]; if (!cnt) continue;
            const int32_t* p = (const int32_t*)(uintptr_t)lBase[l] + lPos[l];
            for (uint32_t i = tid; i < cnt; i += P2_THREADS) sBuf[part[l] + i] = p[i];
        }
        __syncthreads();
        if ((uint32_t)tid < nL) lPos[tid] += lCnt[tid];
        uint32_t b2 = 2; while (b2 < tot) b2 <<= 1;
        for (uint32_t i = tot + tid; i < b2; i += P2_THREADS) sBuf[i] = 0x7FFFFFFF;
        __syncthreads();
        if (tot > 1) wg_bitonic_i32(sBuf, b2, tid, P2_THREADS);
        for (uint32_t i = tid; i < tot; i += P2_THREADS) {
            const int32_t v = sBuf[i];
            sFlag[i] = ((i == 0 || sBuf[i - 1] != v) && !sorted_contains(sTop, ntop, v)) ? 1 : 0;
        }
        __syncthreads();
        const uint32_t got = wg_scan_flags(sFlag, sPos, tot, part, tid, P2_THREADS);
        for (uint32_t i = tid; i < tot; i += P2_THREADS) if (sFlag[i] && nu + sPos[i] < need) sUniq[nu + sPos[i]] = sBuf[i];
        if (del && lv1 < 0 && ntop < 2u) {
            for (uint32_t i = tid; i < tot; i += P2_THREADS) if (sFlag[i] && !del[sBuf[i]]) atomicMin(&shL0, sBuf[i]);
            __syncthreads();
            for (uint32_t i = tid; i < tot; i += P2_THREADS) if (sFlag[i] && !del[sBuf[i]] && sBuf[i] > shL0) atomicMin(&shL1, sBuf[i]);
            __syncthreads();
            const int32_t a0 = shL0, a1 = shL1;
            if (lv0 < 0) { if (a0 != 0x7FFFFFFF) lv0 = a0; if (a1 != 0x7FFFFFFF) lv1 = a1; }
            else if (a0 != 0x7FFFFFFF) lv1 = a0;
        }
        nu = min(need, nu + got);
        __syncthreads();
    }

    P2P(4);
    // ---- docIndex 0 / 1 = the first two keys in insertion order: Stage-1 docs, then WordMatcher-only ids (ascending) ------
    int32_t f0 = -1, f1 = -1;
    { uint32_t nf = 0;
      for (uint32_t k = 0; k < ntop && nf < 2; k++) { if (nf == 0) f0 = sDoc[k]; else f1 = sDoc[k]; nf++; }
      if (!del) { for (uint32_t k = 0; k < nu && nf < 2; k++) { if (nf == 0) f0 = sUniq[k]; else f1 = sUniq[k]; nf++; } }
      else { if (nf < 2 && lv0 >= 0) { if (nf == 0) f0 = lv0; else f1 = lv0; nf++; } if (nf < 2 && lv1 >= 0) { if (nf == 0) f0 = lv1; else f1 = lv1; nf++; } } }
    M.idx0 = f0; M.idx1 = f1;
    uint32_t nWm = min(nu, wmLimit);
    for (uint32_t i = tid; i < nOv; i += P2_THREADS) { const int32_t d = myC[i].doc; if (d == f0 || d == f1) myC[i].want_lcs = 1; }
    if (!del) {
        for (uint32_t i = tid; i < nWm; i += P2_THREADS) { infx_cov_cand cc; cc.query = (uint32_t)qi; cc.doc = sUniq[i]; cc.base_score = 0.f; cc.want_lcs = (cc.doc == f0 || cc.doc == f1) ? 1 : 0; myC[nOv + i] = cc; }
    } else {                                    // the first wmLimit ids were "processed"; only the live ones become candidate rows, in the same order
        __syncthreads();
        for (uint32_t i = tid; i < nWm; i += P2_THREADS) sFlag[i] = del[sUniq[i]] ? 0 : 1;
        __syncthreads();
        const uint32_t nLive = wg_scan_flags(sFlag, sPos, nWm, part, tid, P2_THREADS);
        for (uint32_t i = tid; i < nWm; i += P2_THREADS) if (sFlag[i]) { infx_cov_cand cc; cc.query = (uint32_t)qi; cc.doc = sUniq[i]; cc.base_score = 0.f; cc.want_lcs = (cc.doc == f0 || cc.doc == f1) ? 1 : 0; myC[nOv + sPos[i]] = cc; }
        nWm = nLive;
    }
    const float maxT = ntop ? sScore[0] : 1.f;
    for (uint32_t i = tid; i < ntop; i += P2_THREADS) {
        infx_cov_cand cc; cc.query = (uint32_t)qi; cc.doc = sDoc[i]; cc.base_score = maxT > 0.f ? sScore[i] / maxT : 0.f; cc.want_lcs = (cc.doc == f0 || cc.doc == f1) ? 1 : 0;
        myC[nOv + nWm + i] = cc;
    }
    M.candCount = nOv + nWm + ntop;
    // An overlap document occurs twice: as a WordMatcher row (base 0) and as its Stage-1 row (base = score / top1).  The coverage
    // features do not depend on the base score, so k_stage2 evaluates the document once (on the overlap row) and derives both rows:
    // pairs[overlap row] = its Stage-1 row, pairs[that Stage-1 row] = -2 (skipped).
    __syncthreads();
    for (uint32_t k = tid; k < ntop && nOv > 0; k += P2_THREADS) {
        const int32_t d = sDoc[k];
        uint32_t lo = 0, hi = nOv;
        while (lo < hi) { uint32_t m = (lo + hi) >> 1; if (myC[m].doc < d) lo = m + 1; else hi = m; }
        if (lo < nOv && myC[lo].doc == d) { myP[lo] = (int32_t)((size_t)qi * stride + nOv + nWm + k); myP[nOv + nWm + k] = -2; }     // global row index
    }
    // Stage-2 traffic accounting: UTF-16 bytes of the candidate texts
    __syncthreads();
    if (tid == 0) { shA = 0; shB = 0; }
    __syncthreads();
    { unsigned long long tb = 0;
      for (uint32_t i = tid; i < M.candCount; i += P2_THREADS) { const int32_t d = myC[i].doc - ix.docBase; if (d >= 0 && d < ix.N) tb += 2ull * (ix.textOff[d + 1] - ix.textOff[d]); }
      atomicAdd(&shA, (uint32_t)(tb & 0xFFFFFFFFull)); atomicAdd(&shB, (uint32_t)(tb >> 32)); /* per-thread sums stay far below 2^32 */ }
    __syncthreads();
    if (tid == 0) { M.pad0 = shA; M.pad1 = shB; metas[qi] = M; }
    P2P(5);
}

// ---- k_finalize: one workgroup per query ------------------------------------------------------------------------------------
// dynamic LDS (Cp = power of two >= 2 * depth): sKey[Cp] i64 | sBits[Cp] u32 (score bits) | sPos[Cp] u32 | sIdx[Cp] u16 | sTie[Cp] u8 |
//                                               sFlag[Cp] u8 | part[257] u32
// WIN (k_finalize_win, a batch with a collapsing query): a query with a window (winSlot[qi] >= 0) gets a budget of `depth` rows — its whole ranked list — and
// writes them, documents included, into its window instead of its rows of the batch buffers (collapse.hip.inc).  The other queries of the batch, and every
// query of k_finalize, are written as ever.
struct FinalizeWindows { const int32_t* slot; long long* keys; float* scores; uint8_t* ties; int32_t* docs; };
template <bool WIN> __device__ __forceinline__ void finalize_rows(const DevIndex& ix, const infx_fused_query* __restrict__ fqs, const FusedMeta* __restrict__ metas,
                                                          const infx_cov_cand* __restrict__ cands, const infx_cov_out* __restrict__ outs,
                                                          const infx_hit* __restrict__ s1, int depth, int Cp, int maxResults,
                                                          long long* __restrict__ outKeys, float* __restrict__ outScores, uint8_t* __restrict__ outTies,
                                                          uint32_t* __restrict__ outCounts, uint32_t* __restrict__ outFlags, uint32_t* __restrict__ errFlag,
                                                          int32_t* __restrict__ outDocs, const infx_finalize_setup* __restrict__ fins, const FinalizeWindows& win) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    long long* sKey = (long long*)smem;
    uint32_t* sBits = (uint32_t*)(sKey + Cp);
    uint32_t* sPos = sBits + Cp;
    uint16_t* sIdx = (uint16_t*)(sPos + Cp);
    uint8_t* sTie = (uint8_t*)(sIdx + Cp);
    uint8_t* sFlag = sTie + Cp;
    uint32_t* part = (uint32_t*)(sFlag + Cp);
    __shared__ int shMaxHits, shTrunc; __shared__ uint32_t shFirst[4], shBad;

    const int qi = blockIdx.x, tid = threadIdx.x;
    const infx_fused_query FQ = fqs[qi];
    const FusedMeta M = metas[qi];
    const int32_t ws = WIN ? win.slot[qi] : -1;
    const int mr = ws >= 0 ? depth : min(FQ.max_results, maxResults);
    uint32_t flags = (FQ.flags & FQ_UNSUPPORTED) ? 1u : 0u;
    long long* oK = outKeys + (size_t)qi * maxResults; float* oS = outScores + (size_t)qi * maxResults; uint8_t* oT = outTies ? outTies + (size_t)qi * maxResults : nullptr;
    int32_t* oD = outDocs ? outDocs + (size_t)qi * maxResults : nullptr;       // global internal ids of the rows (post-filter / facets)
    if (ws >= 0) { const size_t w = (size_t)ws * depth; oK = win.keys + w; oS = win.scores + w; oT = win.ties + w; oD = win.docs + w; }
    bool useStage1 = true;
    uint32_t nOut = 0;
    if (M.runCov) {
        flags |= 2u;
        const uint32_t n = M.candCount;
        const infx_cov_cand* C = cands + (size_t)qi * 2u * depth; const infx_cov_out* O = outs + (size_t)qi * 2u * depth;
        if (tid == 0) { shMaxHits = 0; shTrunc = -1; shFirst[0] = shFirst[1] = shFirst[2] = shFirst[3] = 0xFFFFFFFFu; shBad = 0; }
        __syncthreads();
        int mh = 0;
        for (uint32_t i = tid; i < (uint32_t)Cp; i += P2_THREADS) {
            if (i < n) {
                const infx_cov_out o = O[i]; const int32_t d = C[i].doc;
                // a candidate outside the Stage-2 envelope (INFX_MAX_DOC_TOKENS / token length) is not scored: it is left out of THIS query's ranking
                // and the query is flagged (bit 3) — the rest of the batch is unaffected
                if (o.status) { atomicAdd(&shBad, 1u); atomicOr(errFlag, 1u); sKey[i] = 0x7FFFFFFFFFFFFFFFll; sBits[i] = 0; sTie[i] = 0; sIdx[i] = (uint16_t)i; continue; }
                mh = max(mh, (int)o.word_hits_full);
                sKey[i] = ix.docKeyAll[d]; sBits[i] = __float_as_uint(o.score); sTie[i] = o.tiebreaker;
                // word hits / LCS of the docIndex-0/1 documents: the first non-zero value in candidate order
                if (d == M.idx0) { if (o.word_hits) atomicMin(&shFirst[0], i); if (o.lcs) atomicMin(&shFirst[1], i); }
                if (d == M.idx1) { if (o.word_hits) atomicMin(&shFirst[2], i); if (o.lcs) atomicMin(&shFirst[3], i); }
            } else { sKey[i] = 0x7FFFFFFFFFFFFFFFll; sBits[i] = 0; sTie[i] = 0; }
            sIdx[i] = (uint16_t)i;
        }
        if (mh) atomicMax(&shMaxHits, mh);
        __syncthreads();
        const int maxWordHits = shMaxHits;
        const uint32_t nBad = shBad;
        if (nBad) flags |= 8u;
        const int hits0 = shFirst[0] != 0xFFFFFFFFu ? O[shFirst[0]].word_hits : 0, lcs0 = shFirst[1] != 0xFFFFFFFFu ? O[shFirst[1]].lcs : 0;
        const int hits1 = shFirst[2] != 0xFFFFFFFFu ? O[shFirst[2]].word_hits : 0, lcs1 = shFirst[3] != 0xFFFFFFFFu ? O[shFirst[3]].lcs : 0;
        uint32_t ncons = 0;
        if (!(maxWordHits == 0 && !M.wmAny) && n > 0) {
            // ScoreEntry order: score desc, tiebreaker desc, key asc (pad entries last)
            uint32_t n2 = 2; while (n2 < n) n2 <<= 1;
            if (n > 1) wg_bitonic_idx(sIdx, n2, tid, P2_THREADS, [&](uint16_t a, uint16_t b) {
                const bool pa = a >= n || sKey[a] == 0x7FFFFFFFFFFFFFFFll, pb = b >= n || sKey[b] == 0x7FFFFFFFFFFFFFFFll; if (pa != pb) return pb; if (pa) return false;
                if (sBits[a] != sBits[b]) return __uint_as_float(sBits[a]) > __uint_as_float(sBits[b]);
                if (sTie[a] != sTie[b]) return sTie[a] > sTie[b];
                return sKey[a] < sKey[b]; });
            const uint32_t nf = min(n - nBad, (uint32_t)depth); // TopKHeap(depth) over the scored rows
            // ConsolidateSegments: the best entry per key = the first occurrence in sorted order
            for (uint32_t i = tid; i < nf; i += P2_THREADS) {
                const long long k = sKey[sIdx[i]]; uint8_t first = 1;
                for (uint32_t j = 0; j < i; j++) if (sKey[sIdx[j]] == k) { first = 0; break; }
                sFlag[i] = first;
            }
            __syncthreads();
            ncons = wg_scan_flags(sFlag, sPos, nf, part, tid, P2_THREADS);
            // CalculateTruncationIndex: last consolidated row that has enough word hits / an LCS / a near-perfect score
            const infx_finalize_setup FS = fins[qi];      // Truncate, CoverageMinWordHitsAbs / Relative, TruncationScore of this query (ResultProcessor.cs:151-171)
            const int minHits = max(FS.min_hits_abs, maxWordHits - FS.min_hits_relative);
            const float truncScore = (float)FS.truncation_score;
            const long long k0 = M.idx0 >= 0 ? ix.docKeyAll[M.idx0] : (long long)0x8000000000000000ull;
            const long long k1 = M.idx1 >= 0 ? ix.docKeyAll[M.idx1] : (long long)0x8000000000000000ull;
            int myTr = -1;
            for (uint32_t i = tid; i < nf; i += P2_THREADS) if (sFlag[i]) {
                const uint16_t s = sIdx[i]; int wh = 0, lc = 0;
                if (M.idx0 >= 0 && sKey[s] == k0) { wh = hits0; lc = lcs0; }
                else if (M.idx1 >= 0 && sKey[s] == k1) { wh = hits1; lc = lcs1; }
                if (wh >= minHits || lc > 0 || __uint_as_float(sBits[s]) >= truncScore) myTr = max(myTr, (int)sPos[i]);
            }
            if (myTr >= 0) atomicMax(&shTrunc, myTr);
            __syncthreads();
            const int truncIdx = FS.truncate ? shTrunc : -1;      // !Truncate: the full MaxNumberOfRecordsToReturn rows (SearchPipeline.cs:425,433)
            const int resultCount = truncIdx == -1 ? mr : min(truncIdx + 1, mr);
            ncons = min(ncons, (uint32_t)max(0, resultCount));
            if (ncons > 0) {
                useStage1 = false; nOut = min(ncons, (uint32_t)mr);
                for (uint32_t i = tid; i < nf; i += P2_THREADS) if (sFlag[i] && sPos[i] < nOut) {
                    const uint16_t s = sIdx[i]; oK[sPos[i]] = sKey[s]; oS[sPos[i]] = __uint_as_float(sBits[s]); if (oT) oT[sPos[i]] = sTie[s]; if (oD) oD[sPos[i]] = C[s].doc;
                }
            }
        }
        if (useStage1 && M.s1Count > 0) flags |= 4u;       // coverage returned nothing: Stage-1 fallback (SearchPipeline.cs:152-160)
        if (useStage1 && M.s1Count == 0) nOut = 0;
    }
    if (useStage1) {
        nOut = min(M.s1Count, (uint32_t)mr);
        for (uint32_t i = tid; i < nOut; i += P2_THREADS) { const infx_hit h = s1[(size_t)qi * depth + i]; oK[i] = ix.docKeyAll[h.doc]; oS[i] = h.score; if (oT) oT[i] = 0; if (oD) oD[i] = h.doc; }
    }
    if (tid == 0) { outCounts[qi] = nOut; if (outFlags) outFlags[qi] = flags; }
}
#define FINALIZE_PARAMS DevIndex ix, const infx_fused_query* __restrict__ fqs, const FusedMeta* __restrict__ metas, const infx_cov_cand* __restrict__ cands,                       \
                        const infx_cov_out* __restrict__ outs, const infx_hit* __restrict__ s1, int depth, int Cp, int maxResults, long long* __restrict__ outKeys,                 \
                        float* __restrict__ outScores, uint8_t* __restrict__ outTies, uint32_t* __restrict__ outCounts, uint32_t* __restrict__ outFlags,                            \
                        uint32_t* __restrict__ errFlag, int32_t* __restrict__ outDocs, const infx_finalize_setup* __restrict__ fins
#define FINALIZE_ARGS ix, fqs, metas, cands, outs, s1, depth, Cp, maxResults, outKeys, outScores, outTies, outCounts, outFlags, errFlag, outDocs, fins
__global__ __launch_bounds__(P2_THREADS) void k_finalize(FINALIZE_PARAMS) { finalize_rows<false>(FINALIZE_ARGS, FinalizeWindows{}); }
__global__ __launch_bounds__(P2_THREADS) void k_finalize_win(FINALIZE_PARAMS, FinalizeWindows win) { finalize_rows<true>(FINALIZE_ARGS, win); }
