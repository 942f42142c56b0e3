// k_accumulate_sparse — Stage-1 accumulation of the SPARSE (query, stripe) pairs (round 6).  Included by infidex_hip.hip behind stage1.hip.inc; same inputs, same
// arena contract (rows of a (query, range) contiguous and ascending by doc id, directory entry per range, class histogram, hit masks, exception records), same
// arithmetic in the same order as k_accumulate: bit-identical (tests/test_gpu_parity.py::test_accumulate_schedules_agree_bit_for_bit runs every split).
//
// Why a second kernel.  Per 1000-query launch at 10 M documents 59 % of the (query, stripe of 4 ranges) pairs hold <= 64 candidates — 18 on average, 4-5 per range —
// and 5 % of all candidates (profiles/r06_accumulate_search.md); k_accumulate streams every posting of every list through its byte table there (13.7 k postings per
// stripe, ~80 visits of ~100 VALU) to find ~180 (candidate, list) hits: 40 % of its visits.  Here the candidates look their postings up instead
// (MMapBlockPostingsEnum.Advance, :164 — directory entry, then a search inside the block): one wave per (query, stripe); candidate bitmap of the whole stripe in LDS
// from the generating lists; a stripe with more than `denseT` candidates is left to k_accumulate through a flag byte per (query, stripe); otherwise the candidates
// are taken 64 at a time and every (list, candidate) PAIR gets a lane: sixteen evenly spaced postings of every non-empty stripe slice (two skip-table entries bound
// it) are sampled into LDS, the pair finds its sixteenth there and finishes with a branch-free binary search in global memory for the last posting <= the
// candidate's doc id, U passes of 64 pairs side by side; the tf bytes found meet in an LDS matrix and every candidate lane applies its row in Bm25Scorer order.
// (The same lookups for EVERY stripe, candidates one per lane and list after list, took 9.9 ms per launch — the dense stripes' 64 M candidates are what the byte
// table is for.)  Pair of kernels: 7.2 -> ~6.0 ms per launch.
#define ACCS_U 6                       // passes of 64 (candidate, list) pairs searched side by side (independent load chains; a pass keeps three registers: position, length,
                                       // first posting of the part still searched).  Same box, sparse kernel alone: U = 2 without the slice samples 2.63 ms, U = 4 2.34, U = 2 with
                                       // samples 2.24, U = 4 with samples 2.12-2.13, U = 6 2.08, U = 8 2.09.  A block directory in place of the samples (the header of every 16
                                       // postings, found by binary search among the contiguous headers of the slice, then the block read by four lanes or searched by the pair's
                                       // own lane): 2.58 / 2.43 against 2.14 — the kernel pays per lane-load, not per cache line, and a pair then issues ~11 instead of ~7
                                       // (profiles/r06_accumulate_search.md, "Round 6, third part")

template <int R, int MW>
__global__ __launch_bounds__(WAVE) void k_accumulate_sparse(DevIndex ix, const DevQuery* __restrict__ queries, const DevTerm* __restrict__ terms, const int32_t* __restrict__ extraDocs,
                                                            const int32_t* __restrict__ unionDocs, const uint32_t* __restrict__ unionRange, uint32_t nq, Arena ar, int stripe, int useGrp,
                                                            uint8_t* __restrict__ denseFlag, uint32_t denseT, int nStripes, int maxTl, int dbg) {
    constexpr int U = ACCS_U;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int SW = stripe * (R / 32);                                  // bitmap words of a stripe (stripe: a power of two)
    const int WPL = max(1, SW / WAVE);                                 // lane owns words [lane * WPL, lane * WPL + WPL): contiguous, so slot numbers ascend with the doc id
    const int wsh = 31 - __clz(WPL);                                   // word w lives at sBits[w + (w >> wsh)]: one pad word per lane, so the lanes' strided reads of their own
    const int SWP = (SW + (SW >> wsh) + 3) & ~3;                       // words (stride WPL + 1, odd) fall into different banks
    uint32_t* sBits = (uint32_t*)smem;                                 // SWP: candidate bitmap of the stripe
    uint32_t* sHist = sBits + SWP;                                     // INFX_NCLASS
    uint16_t* sDoc = (uint16_t*)(sHist + INFX_NCLASS);                 // 64: slot -> stripe-local doc
    uint2* sTA = (uint2*)(sDoc + WAVE);                                // 64: address of the k-th non-empty slice of the window
    uint32_t* sTL = (uint32_t*)(sTA + WAVE);                           // 64: its length | host list or device union (searched by the candidate lanes, not the pairs) << 29
    uint8_t* sHit = (uint8_t*)(sTL + WAVE);                            // 64 * maxTl: the tf byte pair (k-th slice, slot c) found, at [k * 64 + c]; 0 = no posting
    uint32_t* sSamp = (uint32_t*)(sHit + (size_t)WAVE * maxTl);        // 16 * maxTl: sixteen evenly spaced postings of the k-th slice (element (j * len) >> 4 at [k * 16 + j])

    const int lane = threadIdx.x;
    // the block -> (query, stripe) map of k_accumulate: XCD b % 8 takes the stripes x, x + 8, ... for all queries
    const uint32_t b = blockIdx.x;
    const uint32_t bt = b >> 3; const uint32_t q = bt % nq; const int sIdx = (int)((bt / nq) * 8u + (b & 7u));
    const int r0 = sIdx * stripe;
    if (r0 >= ix.nRanges) return;
    const int rEnd = min(ix.nRanges, r0 + stripe), nr = rEnd - r0;
    const int32_t base = r0 * R;                                       // shard-local doc id of the stripe's first document
    const int32_t send = min(rEnd * R, ix.N);
    const uint32_t span = (uint32_t)(send - base);
    const DevQuery Q = queries[q];
    const uint8_t* const del = q_deleted(ix, q);                       // the query's Document.Deleted flags, selected once per wave (as in k_accumulate)
    const int mode = Q.mode;
    const int nT = (int)Q.numTerms;
    const DevTerm* T = terms + Q.termOff;
    const int nAnd = Q.nAnd;
    const unsigned long long qb = ar.qBase[q];
    const uint32_t qcap = (uint32_t)(ar.qBase[q + 1] - qb);
    const int nWin = (nT + WAVE - 1) / WAVE;
    const unsigned long long lt = (1ull << lane) - 1;
    unsigned long long myBytes = 0;

    // lane-resident descriptor of term (window * 64 + lane): address and length of its slice inside the stripe; tMeta: isVirtual | group << 8 | ref << 16;
    // tUpd: what a hit adds to the candidate's tier flags (k_accumulate's encoding); tIdf: idf, or 0 for a term the scorer skips
    uint32_t tApLo = 0, tApHi = 0, tLen = 0, tMeta = 0, tUpd = 0x1FFu << 16; float tIdf = 0.f;
    auto load_window = [&](int win) -> bool {                          // returns: my term generates candidates
        const int t = win * WAVE + lane;
        tLen = 0; tApLo = 0; tApHi = 0; tIdf = 0.f; tMeta = 0; tUpd = 0x1FFu << 16;
        bool gen = false;
        if (t < nT) {
            const DevTerm tm = T[t];
            tIdf = tm.idf > 0.f ? tm.idf : 0.f;                         // Bm25Scorer.cs:301-309: terms with idf <= 0 are skipped by the scorer
            uint32_t add = 0, rk1 = 0x1FFu;
            if (mode == INFX_MODE_AND) {
                add = ((tm.role & INFX_ROLE_AND) ? 1u : 0u) | ((tm.role & INFX_ROLE_LOWEST) ? F_LOWEST : 0u) | ((tm.role & INFX_ROLE_S1) ? F_S1 : 0u) | ((tm.role & INFX_ROLE_S2) ? F_S2 : 0u);
                gen = (tm.role & (INFX_ROLE_S1 | INFX_ROLE_S2)) != 0;
            } else if (mode == INFX_MODE_DISJ && (tm.role & (INFX_ROLE_ELIGIBLE | INFX_ROLE_LOWQ))) { rk1 = (uint32_t)tm.rank + 1u; gen = true; }
            tUpd = add | (rk1 << 16);
            tMeta = (uint32_t)tm.isVirtual | ((uint32_t)tm.pad << 8) | ((uint32_t)tm.refIdx << 16);
            uint32_t lo, hi;
            if (tm.isVirtual & 4) { lo = unionRange[tm.skip + r0]; hi = unionRange[tm.skip + rEnd]; }
            else if (tm.skip != 0xFFFFFFFFu) { lo = ix.skipTbl[tm.skip + r0]; hi = ix.skipTbl[tm.skip + rEnd]; }
            else {
                const int32_t* arr = (tm.isVirtual & 1) ? extraDocs : ix.postDoc;
                const int pk = (tm.isVirtual & 5) ? 0 : ix.packed;
                lo = (uint32_t)(lower_bound_post(arr, tm.begin, tm.end, base, pk) - tm.begin);
                hi = (uint32_t)(lower_bound_post(arr, tm.begin + lo, tm.end, send, pk) - tm.begin);
            }
            tLen = hi - lo;
            const int32_t* dp = ((tm.isVirtual & 4) ? unionDocs : ((tm.isVirtual & 1) ? extraDocs : ix.postDoc)) + (tm.begin + lo);
            const unsigned long long ap = (unsigned long long)(uintptr_t)dp;
            tApLo = (uint32_t)ap; tApHi = (uint32_t)(ap >> 32);
            myBytes += (unsigned long long)tLen * (tm.isVirtual ? 4u : 5u);
        }
        return gen;
    };

    // ---- slices + candidate bitmap of the stripe -------------------------------------------------------------------------------------
    unsigned long long psBase = 0; uint32_t psLen = 0;                 // the query's prefix DocSet inside the stripe
    if (Q.prefixSet >= 0) {
        const uint64_t pb = ix.psOff[Q.prefixSet], pe = ix.psOff[Q.prefixSet + 1];
        const uint32_t sk = ix.psSkip[Q.prefixSet];
        uint64_t lo, hi;
        if (sk != 0xFFFFFFFFu) { lo = pb + ix.psSkipTbl[sk + r0]; hi = pb + ix.psSkipTbl[sk + rEnd]; }
        else { lo = lower_bound_i32(ix.psDocs, pb, pe, base); hi = lower_bound_i32(ix.psDocs, lo, pe, send); }
        psBase = lo; psLen = (uint32_t)(hi - lo);
    }
    bool anyGen = (mode == INFX_MODE_PREFIX) && psLen > 0;
    bool bitsClear = false;
    auto set_bit = [&](uint32_t l) { const uint32_t w = l >> 5; atomicOr(&sBits[w + (w >> wsh)], 1u << (l & 31)); };
    auto clear_bits = [&]() { if (!bitsClear) { for (int i = lane * 4; i < SWP; i += WAVE * 4) *(uint4*)(sBits + i) = make_uint4(0, 0, 0, 0); bitsClear = true; } };
    // A stripe in which ONE candidate-generating list alone holds more than denseT documents is dense whatever the others add (a list names a document once, and every
    // posting of a generating list is a candidate): handed over before its lists are read — most of the dense stripes, whose bitmaps cost 12 % of this kernel's block time.
    if (mode == INFX_MODE_PREFIX) {
        if (psLen > denseT) { if (lane == 0) denseFlag[(size_t)q * nStripes + sIdx] = 1; return; }
        if (nWin == 1) load_window(0);
        if (anyGen) { clear_bits(); for (uint32_t i = lane; i < psLen; i += WAVE) set_bit((uint32_t)(ix.psDocs[psBase + i] - base)); }
    } else {
        for (int win = 0; win < nWin; win++) {
            const bool gen = load_window(win);
            if (__ballot(gen && tLen > denseT)) { if (lane == 0) denseFlag[(size_t)q * nStripes + sIdx] = 1; return; }
            unsigned long long gm = __ballot(gen && tLen > 0);
            if (gm) { anyGen = true; clear_bits(); }
            while (gm) {
                const int tl = __ffsll((long long)gm) - 1; gm &= gm - 1;
                const uint32_t len = rdl_u(tLen, tl), iv = rdl_u(tMeta, tl) & 0xFFu;
                const unsigned long long ap = ((unsigned long long)rdl_u(tApHi, tl) << 32) | rdl_u(tApLo, tl);
                const int pk = (iv & 5) ? 0 : ix.packed;               // host lists / device unions hold plain doc ids
                if (!(iv & 1)) {
                    // index lists and device unions are 16-byte aligned and sentinel padded: 16-byte loads from the boundary below the slice (elements outside the
                    // slice are postings of other stripes or sentinels: the range check drops them)
                    const uint32_t mis = (uint32_t)((ap >> 2) & 3u);
                    const gint4p ap4 = (gint4p)(uintptr_t)(ap - 4ull * mis);
                    const uint32_t total = len + mis;
                    for (uint32_t i = (uint32_t)lane * 4u; i < total; i += 4u * WAVE) {
                        const int4 c = ld4(ap4, i >> 2);
                        const uint32_t l0 = (uint32_t)post_doc(c.x, pk) - (uint32_t)base, l1 = (uint32_t)post_doc(c.y, pk) - (uint32_t)base;
                        const uint32_t l2 = (uint32_t)post_doc(c.z, pk) - (uint32_t)base, l3 = (uint32_t)post_doc(c.w, pk) - (uint32_t)base;
                        if (l0 < span) set_bit(l0);
                        if (l1 < span) set_bit(l1);
                        if (l2 < span) set_bit(l2);
                        if (l3 < span) set_bit(l3);
                    }
                } else {
                    const gint32p dp = (gint32p)(uintptr_t)ap;
                    for (uint32_t i = lane; i < len; i += WAVE) set_bit((uint32_t)(post_doc(dp[i], pk) - base));
                }
            }
        }
    }
    uint32_t ncand = 0, cnt = 0, incl = 0;
    if (anyGen) {
        for (int j = 0; j < WPL; j++) { const int wi = lane * WPL + j; if (wi < SW) cnt += __popc(sBits[wi + lane]); }
        incl = cnt;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) { const uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }
        ncand = rdl_u(incl, WAVE - 1);
    }
    if (ncand > denseT) {                                              // a dense stripe: left to k_accumulate (byte scatter + probe per range), which counts its bytes itself
        if (lane == 0) denseFlag[(size_t)q * nStripes + sIdx] = 1;
        return;
    }
    if (dbg & 2) ncand = 0;                                            // (profiling ablation: classification only)
    if (ncand) {
        for (int i = lane; i < INFX_NCLASS; i += WAVE) sHist[i] = 0;
        uint32_t chunkOffV = 0;                                        // the stripe's slot block in the query's arena region (the atomic's round trip overlaps the term loop)
        if (lane == 0) chunkOffV = atomicAdd(&ar.qCursor[q], ncand);
        uint32_t chunkOff = 0; unsigned long long outBase = 0; bool haveOff = false, dropped = false;
        uint32_t written = 0, rCnt = 0, myMax = 0;                     // rCnt: lane k < nr counts the rows emitted for range r0 + k
        for (uint32_t rb = 0; rb < ncand && !dropped; rb += WAVE) {    // rounds of 64 candidates (stripes beyond 64 candidates: every round searches every list again)
        const uint32_t nslot = min((uint32_t)WAVE, ncand - rb);
        {                                                              // slot -> doc of this round
            uint32_t sl = incl - cnt;
            if (sl < rb + nslot && incl > rb)
                for (int j = 0; j < WPL; j++) {
                    const int wi = lane * WPL + j;
                    uint32_t bits = wi < SW ? sBits[wi + lane] : 0u;
                    while (bits) { const int bpos = __ffs(bits) - 1; bits &= bits - 1; const uint32_t rel = sl - rb; if (rel < nslot) sDoc[rel] = (uint16_t)(wi * 32 + bpos); sl++; }
                }
        }
        // candidate state, one candidate per lane
        const bool valid = (uint32_t)lane < nslot;
        const uint32_t cDoc = valid ? (uint32_t)sDoc[lane] : 0u;       // stripe-local doc id
        const uint32_t docS = (uint32_t)base + cDoc;                   // shard-local doc id
        const float cNorm = valid ? ix.docNorm[docS] : 1.0f;
        float cAcc = 0.f; uint32_t cFlag = 0, cRank = 0x1FFu, cGrp = 0, cExc = 0; unsigned long long cMask[MW];
#pragma unroll
        for (int w = 0; w < MW; w++) cMask[w] = 0ull;

        struct TermS { uint32_t meta, upd; float idf; };
        // BM25+ update by one list for the lanes that found their own document in it (tfb: its tf byte, 0 = no posting)
        auto apply = [&](const TermS& S, uint32_t tfb) {
            const uint32_t iv = S.meta & 0xFFu, grp = (S.meta >> 8) & 0xFFu, ref = S.meta >> 16;
            const bool unit = iv != 0;                                 // virtual term: tf == 1 (RoaringPostingsEnum.cs:21)
            if (!__ballot(tfb != 0)) return;
            if (grp && useGrp) { const bool dup = cGrp == grp; if (tfb) cGrp = grp; if (dup) tfb = 0; }   // union semantics of ExpandMissingTerm (VectorModel.cs:722-731)
            const bool hit = tfb != 0;
            {
                const float tf = unit ? 1.0f : (float)tfb;
                const float denom = tf + cNorm;
                const float core = (tf * (1.2f + 1.0f)) / denom;       // (tf * (K1 + 1)) / (tf + normFactor)
                const float sc = S.idf * (core + 1.0f);                // idf * (bm25Core + Delta); idf == 0 for a term the scorer skips
                cAcc += hit ? sc : 0.f;
            }
            const uint32_t addFlag = S.upd & 0xFFFFu, rk1 = S.upd >> 16;
            cFlag += hit ? addFlag : 0u;
            cRank = min(cRank, hit ? rk1 : 0x1FFu);
            if (ar.maskWords != 0 && ref < 32u * (uint32_t)MW) {
                const uint32_t capCode = unit ? 1u : 3u;              // hit-mask code: 1 (tf 1 / virtual), 2, 3 (tf >= 3)
                const unsigned long long code = (unsigned long long)min(tfb, capCode) << ((ref & 31u) * 2u);
                const uint32_t wsel = ref >> 5;
#pragma unroll
                for (int w = 0; w < MW; w++) if (wsel == (uint32_t)w) cMask[w] |= code;
                if (!unit && __ballot(tfb >= 3u)) {                    // keep the exact tf beside the 2-bit code
                    const uint32_t rec = ((ref + 1u) << 8) | tfb;
                    if (tfb >= 3u) { if (!(cExc & 0xFFFFu)) cExc |= rec; else if (!(cExc >> 16)) cExc |= rec << 16; }
                }
            }
        };
        // Lanes = (list, candidate) PAIRS.  The nslot candidates of the round times the window's non-empty slices, list-major, 64 pairs per pass (whole lists: 64 /
        // nslot of them), U passes side by side: every lane searches ITS slice for ITS candidate — branch-free, for the LAST posting <= the candidate's doc id, the
        // trip count of the longest slice in flight — and leaves the tf byte it finds in sHit[list][candidate].  All lists of a candidate are searched at once instead
        // of one after the other: the dependent-load chain of a stripe is ~log2(slice) * passes / U long, not ~log2(slice) * lists.  Then every candidate lane
        // applies its row of sHit in Bm25Scorer order (ascending termId): the accumulation order is the reference's.
        const uint32_t tpp = (uint32_t)WAVE / nslot;                   // lists per pass
        const uint32_t mdiv = (65536u + nslot - 1u) / nslot;           // lane / nslot == (lane * mdiv) >> 16 for lane < 64
        const uint32_t kl = ((uint32_t)lane * mdiv) >> 16, cl = (uint32_t)lane - kl * nslot;       // my list within a pass, my candidate
        const uint32_t pairDoc = (uint32_t)base + (uint32_t)sDoc[cl < nslot ? cl : 0];
        for (int win = 0; win < nWin; win++) {
            if (nWin > 1) load_window(win);
            const unsigned long long tmask = __ballot(tLen > 0);       // the window's non-empty slices, ascending term order
            if (!tmask) continue;
            const uint32_t nLive = (uint32_t)__popcll(tmask);
            if (tLen > 0) {
                const uint32_t k = (uint32_t)__popcll(tmask & lt), iv = tMeta & 0xFFu;
                sTA[k] = make_uint2(tApLo, tApHi); sTL[k] = tLen | ((iv & 5u) ? 1u << 29 : 0u);
            }
            for (uint32_t i = (uint32_t)lane * 4u; i < nLive * (uint32_t)WAVE; i += 4u * WAVE) *(uint32_t*)(sHit + i) = 0u;
            // sixteen samples per slice, four slices per wave-load: the first four levels of every pair's search run in LDS (a pair's search costs ~7 global loads
            // instead of ~11, the samples cost 16 per LIST)
            for (uint32_t i = (uint32_t)lane; i < nLive * 16u; i += WAVE) {
                const uint32_t k = i >> 4, j = i & 15u;
                const uint2 a = sTA[k]; const uint32_t len = sTL[k] & 0x1FFFFFFFu;
                sSamp[i] = ((const uint32_t*)(uintptr_t)(((unsigned long long)a.y << 32) | a.x))[(j * len) >> 4];
            }
            const uint32_t keyP = ix.packed ? ((pairDoc << 8) | 0xFFu) : pairDoc;       // postings compare as stored: (doc << 8) | tf, or plain doc ids
            const uint32_t* const pd = (const uint32_t*)ix.postDoc;
            for (uint32_t k0 = 0; k0 < nLive && !(dbg & 1); k0 += tpp * (uint32_t)U) {
                // per pass: position (index into the shard's postings: 32 bits, launch_acc) and length of the part of the slice that can hold the last posting <= the
                // candidate, and the part's first posting; a pass without a pair (or with a host list / device union, searched below) holds n = 0, xb = ~0
                uint32_t n[U], pos[U], xb[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t kk = k0 + (uint32_t)u * tpp + kl;
                    n[u] = 0; pos[u] = 0; xb[u] = 0xFFFFFFFFu;
                    if (kl < tpp && kk < nLive) {
                        const uint32_t L = sTL[kk];
                        if (!((L >> 29) & 1u)) {
                            const uint2 a = sTA[kk];
                            const uint32_t A = (uint32_t)((const uint32_t*)(uintptr_t)(((unsigned long long)a.y << 32) | a.x) - pd), len = L & 0x1FFFFFFFu;
                            // the last sample <= key (sample 0 when none is: the search below then ends on a posting > key, no hit)
                            const uint32_t* sp = sSamp + kk * 16u;
                            uint32_t j = 0;
#pragma unroll
                            for (uint32_t st = 8; st > 0; st >>= 1) j += (sp[j + st] <= keyP) ? st : 0u;
                            const uint32_t lo = (j * len) >> 4, hi = j == 15u ? len : (((j + 1u) * len) >> 4);
                            pos[u] = A + lo; n[u] = max(hi - lo, 1u); xb[u] = sp[j];
                        }
                    }
                }
                // if a posting <= key exists in the slice, the last such lies in [pos, pos + n); xb = its first posting
                bool more = false;
#pragma unroll
                for (int u = 0; u < U; u++) more = more || n[u] > 1;
                while (__ballot(more)) {
                    uint32_t o[U], x[U];
#pragma unroll
                    for (int u = 0; u < U; u++) { const uint32_t half = n[u] >> 1; o[u] = pos[u] + half; x[u] = (n[u] > 1) ? pd[o[u]] : xb[u]; n[u] -= half; }
                    more = false;
#pragma unroll
                    for (int u = 0; u < U; u++) { const bool le = x[u] <= keyP; pos[u] = le ? o[u] : pos[u]; xb[u] = le ? x[u] : xb[u]; more = more || n[u] > 1; }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (ix.packed ? (xb[u] >> 8) == pairDoc : xb[u] == pairDoc) {          // (~0 matches no document: doc ids stay below 2^24 - 1 packed, 2^31 plain)
                        const uint32_t tfb = ix.packed ? (xb[u] & 0xFFu) : (uint32_t)ix.postW[pos[u]];      // unpacked index (shards of >= 2^24 - R documents): tf from the byte array
                        sHit[(k0 + (uint32_t)u * tpp + kl) * (uint32_t)WAVE + cl] = (uint8_t)tfb;
                    }
                }
            }
            // host-supplied lists and device unions (plain doc ids, no directory; rare): every candidate lane searches them itself, one list after the other
            for (unsigned long long lm = (dbg & 1) ? 0ull : __ballot((uint32_t)lane < nLive && ((sTL[lane] >> 29) & 1u)); lm; lm &= lm - 1) {
                const uint32_t kL = (uint32_t)__ffsll((long long)lm) - 1u;
                const uint2 a = sTA[kL]; const uint32_t len = sTL[kL] & 0x1FFFFFFFu;
                const uint32_t* lp = (const uint32_t*)(uintptr_t)(((unsigned long long)a.y << 32) | a.x);
                if (valid) {
                    uint32_t lo = 0, hi = len;                                              // first element >= my document
                    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (lp[m] < docS) lo = m + 1u; else hi = m; }
                    if (lo < len && lp[lo] == docS) sHit[kL * (uint32_t)WAVE + (uint32_t)lane] = (uint8_t)1u;      // (such lists count every document once)
                }
            }
            // my row of sHit, list by list
            uint32_t k = 0;
            for (unsigned long long tm = (dbg & 4) ? 0ull : tmask; tm; tm &= tm - 1, k++) {
                const int tl = __ffsll((long long)tm) - 1;
                TermS S; S.meta = rdl_u(tMeta, tl); S.upd = rdl_u(tUpd, tl); S.idf = rdl_f(tIdf, tl);
                apply(S, valid ? (uint32_t)sHit[k * (uint32_t)WAVE + (uint32_t)lane] : 0u);
            }
        }
        // ---- classify + count + compact -----------------------------------------------------------------------------------------
        if (!haveOff) {
            chunkOff = (uint32_t)rfl_i((int)chunkOffV); haveOff = true;
            if (chunkOff + ncand > qcap) { if (lane == 0) atomicExch(ar.overflow, 1u); dropped = true; }
            outBase = qb + chunkOff;
        }
        if (!dropped) {
            bool emit = false; uint8_t cls = 0; const float sc = cAcc; const uint32_t f = (mode == INFX_MODE_DISJ) ? (cRank == 0x1FFu ? 0u : cRank) : cFlag;
            if (valid && sc > 0.f) {
                if (mode == INFX_MODE_AND) {
                    if (f & (F_S1 | F_S2)) {
                        emit = true;
                        const int c2 = (int)(f & 0xFF);
                        const bool t1 = c2 == nAnd - 1;               // contains terms[0..n-2]
                        const bool t0b = t1 && (f & F_LOWEST);        // ... and the lowest-IDF term: Tier 0
                        cls = (uint8_t)((t0b ? 1 : 0) | ((t1 && nAnd >= 3) ? 2 : 0) | ((f & F_S1) ? 4 : 0) | ((f & F_S2) ? 8 : 0));
                        atomicAdd(&sHist[cls], 1u);
                    }
                } else if (mode == INFX_MODE_DISJ) {
                    if (f != 0) {
                        emit = true;
                        cls = (uint8_t)((f - 1) & 0x7F);
                        bool pre = false;                            // pre-"seen" docs do not count towards localCount (:74-77, :283)
                        if (psLen) {
                            const int32_t d = (int32_t)docS;
                            const uint64_t p = lower_bound_i32(ix.psDocs, psBase, psBase + psLen, d);
                            pre = p < psBase + psLen && ix.psDocs[p] == d;
                        }
                        if (pre) cls |= 0x80; else atomicAdd(&sHist[cls], 1u);
                    }
                } else { emit = true; cls = 1; atomicAdd(&sHist[1], 1u); }
            }
            const unsigned long long m = __ballot(emit);
            if (emit) {
                const unsigned long long pos = outBase + written + __popcll(m & lt);
                ar.doc[pos] = ix.docBase + (int32_t)docS;
                const float stored = (del && del[ix.docBase + (int32_t)docS]) ? 0.f : sc;      // Document.Deleted (Bm25Scorer.cs:322-323): the row stays, with score 0
                ar.score[pos] = stored; myMax = max(myMax, __float_as_uint(stored));
                ar.cls[pos] = cls;
                if (ar.maskWords) {
#pragma unroll
                    for (int w = 0; w < MW; w++) ar.mask[pos * (unsigned long long)MW + w] = cMask[w];
                    ar.exc[pos] = cExc;
                }
            }
            written += (uint32_t)__popcll(m);
            // rows per range: the emitted rows ascend by doc id, so the rows of a range are consecutive
            const uint32_t rng = cDoc / (uint32_t)R;
#pragma unroll 1
            for (int k = 0; k < nr; k++) { const uint32_t c = (uint32_t)__popcll(__ballot(emit && rng == (uint32_t)k)); if (lane == k) rCnt += c; }
        }
        }   // rounds
        if (haveOff && !dropped) {
            uint32_t rIncl = rCnt;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) { const uint32_t v = __shfl_up(rIncl, d); if (lane >= d) rIncl += v; }
            if (lane < nr && rCnt) ar.dir[(unsigned long long)q * ix.nRanges + r0 + lane] = make_uint2(chunkOff + rIncl - rCnt, rCnt);
            if (lane == 0) myBytes += (unsigned long long)written * 12ull;
            for (uint32_t i = written + lane; i < ncand; i += WAVE) { ar.cls[outBase + i] = CLS_HOLE; ar.score[outBase + i] = 0.f; }     // k_select skips rows with score bits 0
            for (int i = lane; i < INFX_NCLASS; i += WAVE) { const uint32_t c = sHist[i]; if (c) atomicAdd(&ar.counts[(uint64_t)q * INFX_NCLASS + i], c); }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) myMax = max(myMax, (uint32_t)__shfl_down((int)myMax, d));
            if (lane == 0 && myMax) atomicMax(&ar.qMax[q], myMax);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) myBytes += __shfl_down(myBytes, d);
    if (lane == 0 && myBytes) atomicAdd(&ar.qBytes[q], myBytes);
}
