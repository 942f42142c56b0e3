// Stage 1 on device: k_accumulate (posting streaming + BM25+ accumulation + tier classification + compaction) and
// k_select (per-query top-`depth`).  Included by infidex_hip.hip.
//
// Replaces Bm25Scorer.ProcessBlockedCandidates / ProcessChunk / ScoreBlockStruct (Indexing/Bm25Scorer.cs:195-445) and
// the data-dependent part of TieredCandidateSelector.SelectCandidates (Scoring/TieredCandidateSelector.cs:128-234,
// 243-322, 328-437).

// per-candidate tier flags (one VGPR per candidate slot)
//   AND : bits 0..7 count of ROLE_AND terms hit, bit 8 LOWEST hit, bit 9 S1, bit 10 S2
//   DISJ: bits 0..7 (min rank + 1), 0 = not hit by a candidate-generating term
#define F_LOWEST 0x100
#define F_S1 0x200
#define F_S2 0x400
#define CLS_HOLE 0xFF       // arena slot reserved for a range but not filled (k_select skips it)

struct Arena {
    int32_t* doc; float* score; uint8_t* cls;
    unsigned long long* mask;          // maskWords u64 per row: 2 bits per reference term (0 no posting, 1 tf==1, 2 tf==2, 3 other tf) — read by the exact replay
    uint32_t* exc;                     // per row: up to two ((term + 1) << 8 | tf) records (low / high half) for the postings with tf >= 3
    const unsigned long long* qBase;   // nq+1: every query owns arena[qBase[q], qBase[q+1]) (host-computed upper bounds) —
    uint32_t* qCursor;                 // nq  : per-query fill counters; a single global cursor would serialise all
    uint32_t* counts;                  // nq * INFX_NCLASS            workgroups on one L2 atomic (~88 M/s on MI355X)
    uint32_t* overflow;                // set to 1 when a region would overflow
    unsigned long long* qBytes;        // nq  : algorithmic bytes streamed per query
    uint32_t* qMax;                    // nq  : best score (bits) among the query's emitted rows, whatever their class — k_select's histogram origin
    uint2* dir;                        // nq * nRanges: {offset relative to qBase[q], rows written} of the (query, range) chunk: the rows of a chunk
                                       // ascend by doc id and ranges ascend, so the directory yields a query's rows in doc order (k_exact1)
    int maskWords;                     // 0 (no masks kept), 1, 2, or 4 (a batch with a query of 65 .. 128 reference terms)
};

#define ACC_WPS 4                     // waves per SIMD the register budget allows (4: 128 VGPRs).  Round 5 measured 3 waves / 168 VGPRs (8.98 ms), a third load in flight
                                      // (8.91 ms), a straight-line probe (7.42 ms) and an own fp32 division without the v_div_scale / v_div_fixup frame (7.15 ms) against 7.14 ms
                                      // as compile-time variants; round 6 a two-pass form (no BM25+ arithmetic in the probe, a second kernel scores the 29 % of the rows that pass
                                      // the tier rule: 6.83 + 1.04 ms against 7.09).  None was adopted and their code is gone (HISTORY.md)
#define ACC_PF 2                      // first loads of the next ACC_PF non-empty lists in flight while a list is scattered and probed
#define ACC_G 2                       // candidate groups of 64 held in registers per round (10 M-doc batch: G = 1: 10.97 ms, 2: 8.62, 3: 8.85, 4: 8.87 —
                                      // ranges average 16 candidates; two groups leave the register file free of spills and room for the scatter below.  Round 6, on the dense stripes
                                      // alone (147 candidates per range, 1.72 rounds): G = 2: 4.05 ms, 3: 4.34 (28-60 B scratch), 4: 4.36)
#define ACC_CAP_DEFAULT (64 * ACC_G)  // candidate slots per round; denser ranges take several rounds

// k_accumulate — one wave per (query, stripe of consecutive doc ranges of R documents); per range:
//   1. lane t holds term t: its DevTerm constants and, per range, its posting slice (skip table / binary search: one L2 round trip for
//      the whole query).  Nothing about a term is fetched again inside the term loop: the loop reads a term's descriptor out of the
//      lanes with v_readlane, and walks the non-empty slices through a ballot mask.  (Queries with more than 64 lists — fuzzy member
//      lists — are handled in windows of 64 terms.)
//   2. the slices of the candidate-GENERATING lists (Tier-2 selective terms S1/S2, the eligible disjunctive terms, or the
//      accepted prefix DocSet) set a candidate bitmap of R bits in LDS; a range without candidates is skipped (range-granular
//      WAND skip).  Only candidates can reach the top-k (TieredCandidateSelector returns a subset of them).
//   3. the candidates (<= 64 * ACC_G per round) are held ONE PER LANE in registers: local doc id, docNorm, fp32 score, tier flags,
//      hit mask.  Every posting slice of the query is then processed in Bm25Scorer order (ascending termId) as
//        scatter : the slice is streamed with 16-byte loads and every posting writes its tf byte to sTf[doc - rangeBase] (LDS, one
//                  ds_write_b8 per posting, no branch: postings outside the range land in a dummy zone);
//        probe   : every candidate lane reads sTf[its doc] — non-zero = the term occurs in the candidate — and adds
//                  idf * (tf * 2.2 / (tf + norm) + 1) to its register accumulator with all hit lanes active;
//        restore : only candidate cells are ever read, so the candidate lane writes 0 back to its own cell right after reading it; the cells
//                  dirtied by non-candidate postings stay dirty until the array is wiped once at the start of the next round (16-byte stores).
//                  (Before: the posting lanes re-scattered zeros after every list — 8.05 -> 7.35 ms per launch when that went.  An earlier
//                  alternative, cells tagged with a 4-bit list generation, lost to the per-posting tag arithmetic: 9.2 vs 8.75 ms.)
//      A posting costs 3 VALU + 1 LDS write whether or not its document is a candidate; the per-hit divergence of a
//      posting-side probe (1-2 active lanes per BM25 update) is gone.  One wave executes its LDS operations in program order, so
//      no barrier or atomic is needed and the per-document accumulation order is the reference's term order (Q8).
//   4. candidates with score > 0 are classified by tier flags, counted and ballot-compacted — in doc order — into the slot block
//      the range reserved in the query's arena region; the (query, range) directory records where.
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) v4i_t* gint4p;        // posting loads through addresses rebuilt from lane registers: global, not flat
__device__ __forceinline__ int4 ld4(gint4p p, uint32_t i) { const v4i_t v = p[i]; return make_int4(v.x, v.y, v.z, v.w); }
typedef const __attribute__((address_space(1))) int32_t* gint32p;
__device__ __forceinline__ uint32_t rdl_u(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float rdl_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// Byte access to the tf array at LDS offset `off`.  k_accumulate has no static __shared__ data, so its dynamic LDS starts at address 0 and sTf[i]
// IS LDS address i: spelling the access as an address-space-3 pointer built from the integer saves the "+ base" VALU add the generic
// smem[] indexing costs per access (13 per list visit).
typedef __attribute__((address_space(3))) uint8_t lds_u8_t;
#define LDS8(off) (*(lds_u8_t*)(uint32_t)(off))

template <int R, int MW>
__global__ __launch_bounds__(WAVE, ACC_WPS) void k_accumulate(DevIndex ix, const DevQuery* __restrict__ queries,
                                                      const DevTerm* __restrict__ terms, const int32_t* __restrict__ extraDocs,
                                                      const int32_t* __restrict__ unionDocs, const uint32_t* __restrict__ unionRange, uint32_t nq, Arena ar, int maxT, int stripe, int useGrp, int dbgSkip, unsigned long long* __restrict__ stats,
                                                      const uint8_t* __restrict__ dense, int nStripes, const uint32_t* __restrict__ qOrder, uint32_t nHeavy) {
    constexpr int W = R / 32;                                          // bitmap words
    constexpr int WPL = (W + WAVE - 1) / WAVE;                         // words per lane (1 for R <= 2048)
    constexpr int G = ACC_G, CAP = WAVE * ACC_G;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint8_t* sTf = (uint8_t*)smem;                                     // [0, R) tf by local doc | [R, R+64) scatter dummies | [R+64, R+128) always zero (probe dummies)
    uint32_t* sBits = (uint32_t*)(sTf + R + 128);                      // W + 2: candidate bitmap
    uint32_t* sHist = sBits + W + 2;                                   // INFX_NCLASS
    uint16_t* sDoc = (uint16_t*)(sHist + INFX_NCLASS);                 // CAP  slot -> local doc of the current round

    const int lane = threadIdx.x;
    // XCD-aware block -> (query, stripe) map.  Block b runs on XCD b % 8 (observed placement, used for speed only): XCD x takes the stripes x, x + 8, ...
    // for ALL queries, one query after the other, so the ~500 waves an XCD holds work on the SAME doc ranges for different queries and the posting
    // slices the queries share (a 1000-query batch reads every distinct slice 8.9 times, INFX_ACC_SHARE_STATS) hit in that XCD's 4 MB L2 instead of
    // being fetched once per query.  (dbgSkip & 32: the old query-fastest order, for A/B runs.)
    const uint32_t b = blockIdx.x;
    uint32_t q; int sIdx;
    if (dbgSkip & 32) { q = b % nq; sIdx = (int)(b / nq); }
    else if (qOrder) {
        // Heaviest queries first (round 6, per-block timestamps: profiles/r06_accumulate_blocks.md): a block of the batch's largest query runs ~1 ms, the mean block
        // 0.13 ms, and in query order such blocks start until the end of the launch — its last 0.6 ms ran with the slots draining (13 % of the launch).  The host orders the
        // queries by their row bound, descending; the first nHeavy of them take ALL their stripes first (stripe fastest), the others follow in the XCD-aware order.
        const uint32_t ns8 = (uint32_t)((nStripes + 7) / 8) * 8u, hb = nHeavy * ns8;
        if (b < hb) { q = qOrder[b / ns8]; sIdx = (int)(b % ns8); }
        else { const uint32_t t = (b - hb) >> 3, nr = nq - nHeavy; q = qOrder[nHeavy + t % nr]; sIdx = (int)((t / nr) * 8u + (b & 7u)); }
    }
    else { const uint32_t t = b >> 3; q = t % nq; sIdx = (int)((t / nq) * 8u + (b & 7u)); }
    if (sIdx * stripe >= ix.nRanges) return;
    if (dense && !dense[(size_t)q * nStripes + (size_t)sIdx]) return;      // behind k_accumulate_sparse (stage1_sparse.hip.inc): only the (query, stripe) pairs that kernel left to this one
    const DevQuery Q = queries[q];
    // The query's Document.Deleted flags (its pre-filter mask, or the index's): selected once per wave, here, so that ONE pointer stays alive across the list
    // loop — inside the emission loop the select keeps the table pointer and the index's flags pointer alive as well (profiles/prefilter.md).
    const uint8_t* const del = q_deleted(ix, q);
    const int mode = Q.mode;
    const int nT = (int)Q.numTerms;
    const DevTerm* T = terms + Q.termOff;
    const int nAnd = Q.nAnd;
    const uint32_t Rlane = (uint32_t)R + (uint32_t)lane;               // scatter address of a posting outside the range
    const unsigned long long qb = ar.qBase[q];
    const uint32_t qcap = (uint32_t)(ar.qBase[q + 1] - qb);
    const int nWin = (nT + WAVE - 1) / WAVE;

    for (int i = lane * 16; i < R + 128; i += WAVE * 16) *(uint4*)(sTf + i) = make_uint4(0, 0, 0, 0);
    for (int i = lane; i < INFX_NCLASS; i += WAVE) sHist[i] = 0;
    unsigned long long myBytes = 0;
    uint32_t myMax = 0;                                                // best emitted score (bits) this lane wrote

    // lane-resident descriptor of term (window * 64 + lane): constants of the term + its slice in the current range
    // tAp: address of the slice's first 16-byte aligned load; tPack: total | mis << 16 | ref << 18 (total = len + mis elements of the aligned
    // stream, mis = elements before the slice); tMeta: isVirtual << 16 | group << 24; tUpd: what a hit adds to the candidate's tier flags
    // (AND mode: 1 for an AND-role term | F_LOWEST | F_S1 | F_S2) | (rank + 1, or 0x1FF for a term that generates no candidates) << 16;
    // tIdf: idf, or 0 for a term the scorer skips (idf <= 0: adding 0.0f leaves the accumulator unchanged)
    uint32_t tApLo = 0, tApHi = 0, tPack = 0, tLen = 0, tMeta = 0, tUpd = 0x1FFu << 16; float tIdf = 0.f;
    uint32_t tRef = 0; bool tGen = false;
    DevTerm tm{}; bool tmValid = false;
    auto load_window_consts = [&](int win) {                           // DevTerm of my term (one 32-byte load per lane)
        const int t = win * WAVE + lane;
        tmValid = t < nT;
        if (tmValid) tm = T[t];
        tIdf = (tmValid && tm.idf > 0.f) ? tm.idf : 0.f;                // Bm25Scorer.cs:301-309: terms with idf <= 0 are skipped by the scorer
        tMeta = tmValid ? (((uint32_t)tm.isVirtual << 16) | ((uint32_t)tm.pad << 24)) : 0u;
        tUpd = 0x1FFu << 16;
        if (tmValid) {
            uint32_t add = 0, rk1 = 0x1FFu;
            if (mode == INFX_MODE_AND) add = ((tm.role & INFX_ROLE_AND) ? 1u : 0u) | ((tm.role & INFX_ROLE_LOWEST) ? F_LOWEST : 0u) | ((tm.role & INFX_ROLE_S1) ? F_S1 : 0u) | ((tm.role & INFX_ROLE_S2) ? F_S2 : 0u);
            else if (mode == INFX_MODE_DISJ && (tm.role & (INFX_ROLE_ELIGIBLE | INFX_ROLE_LOWQ))) rk1 = (uint32_t)tm.rank + 1u;
            tUpd = add | (rk1 << 16);
        }
        tRef = tmValid ? tm.refIdx : 0u;
        tGen = false;
        if (tmValid) {
            if (mode == INFX_MODE_AND) tGen = (tm.role & (INFX_ROLE_S1 | INFX_ROLE_S2)) != 0;
            else if (mode == INFX_MODE_DISJ) tGen = (tm.role & (INFX_ROLE_ELIGIBLE | INFX_ROLE_LOWQ)) != 0;
        }
    };
    auto locate_window = [&](int r, int32_t base, int32_t rend) {      // my term's slice inside the range
        tLen = 0; tApLo = 0; tApHi = 0; tPack = 0;
        if (tmValid) {
            uint32_t lo, hi;
            if (tm.isVirtual & 4) { lo = unionRange[tm.skip + r]; hi = unionRange[tm.skip + r + 1]; }
            else if (tm.skip != 0xFFFFFFFFu) { lo = ix.skipTbl[tm.skip + r]; hi = ix.skipTbl[tm.skip + r + 1]; }
            else {
                const int32_t* arr = (tm.isVirtual & 1) ? extraDocs : ix.postDoc;
                const int pk = (tm.isVirtual & 5) ? 0 : ix.packed;
                lo = (uint32_t)(lower_bound_post(arr, tm.begin, tm.end, base, pk) - tm.begin);
                hi = (uint32_t)(lower_bound_post(arr, tm.begin + lo, tm.end, rend, pk) - tm.begin);
            }
            tLen = hi - lo;
            const int32_t* dp = ((tm.isVirtual & 4) ? unionDocs : ((tm.isVirtual & 1) ? extraDocs : ix.postDoc)) + (tm.begin + lo);
            const uint32_t mis = (uint32_t)(((uintptr_t)dp >> 2) & 3u);             // elements between the 16-byte boundary below the slice and its start
            const unsigned long long ap = (unsigned long long)(uintptr_t)(dp - mis);
            tApLo = (uint32_t)ap; tApHi = (uint32_t)(ap >> 32);
            const bool simple = ix.packed && !tm.isVirtual && !tm.pad && tLen + mis <= 4u * WAVE;      // fast_list's precondition
            tPack = (tLen + mis) | (mis << 16) | (tRef << 18) | (simple ? 0x80000000u : 0u);
            myBytes += (unsigned long long)tLen * (tm.isVirtual ? 4u : 5u);
        }
    };
    if (nWin == 1) load_window_consts(0);

    const int rEnd = min(ix.nRanges, (sIdx + 1) * stripe);
    for (int r = sIdx * stripe; r < rEnd; r++) {
    const int32_t base = r * R;            // shard-local doc id of the range start
    const int32_t rend = min(base + R, ix.N);

    // ---- 1. slices + 2. candidate bitmap --------------------------------------------------------------------------------------
    unsigned long long psBase = 0; uint32_t psLen = 0;                 // the query's prefix DocSet inside the range
    if (Q.prefixSet >= 0) {
        const uint64_t pb = ix.psOff[Q.prefixSet], pe = ix.psOff[Q.prefixSet + 1];
        const uint32_t sk = ix.psSkip[Q.prefixSet];
        uint64_t lo, hi;
        if (sk != 0xFFFFFFFFu) { lo = pb + ix.psSkipTbl[sk + r]; hi = pb + ix.psSkipTbl[sk + r + 1]; }
        else { lo = lower_bound_i32(ix.psDocs, pb, pe, base); hi = lower_bound_i32(ix.psDocs, lo, pe, rend); }
        psBase = lo; psLen = (uint32_t)(hi - lo);
    }
    bool anyGen = (mode == INFX_MODE_PREFIX) && psLen > 0;
    bool bitsClear = false;
    auto clear_bits = [&]() { if (!bitsClear) { for (int i = lane; i < W + 2; i += WAVE) sBits[i] = 0; bitsClear = true; } };
    if (mode == INFX_MODE_PREFIX) {
        if (nWin == 1) locate_window(r, base, rend);
        if (anyGen) { clear_bits(); for (uint32_t i = lane; i < psLen; i += WAVE) { int l = ix.psDocs[psBase + i] - base; atomicOr(&sBits[l >> 5], 1u << (l & 31)); } }
    } else {
        for (int win = 0; win < nWin; win++) {
            if (nWin > 1) load_window_consts(win);
            locate_window(r, base, rend);
            unsigned long long gm = __ballot(tGen && tLen > 0);
            if (gm) { anyGen = true; clear_bits(); }
            while (gm) {
                const int tl = __ffsll((long long)gm) - 1; gm &= gm - 1;
                const uint32_t pack = rdl_u(tPack, tl), iv = (rdl_u(tMeta, tl) >> 16) & 0xFFu;
                const uint32_t mis = (pack >> 16) & 3u, len = (pack & 0xFFFFu) - mis;
                const int pk = (iv & 5) ? 0 : ix.packed;               // host lists / device unions hold plain doc ids
                if (!(iv & 1)) {
                    // index lists and device unions are 16-byte aligned and sentinel padded: 16-byte loads, four postings per lane (elements outside the
                    // slice are postings of other ranges or sentinels: the range check drops them).  In disjunctive mode EVERY eligible list generates
                    // candidates, so this pass streams as many postings as the scoring pass.
                    const gint4p ap4 = (gint4p)(uintptr_t)(((unsigned long long)rdl_u(tApHi, tl) << 32) | rdl_u(tApLo, tl));
                    const uint32_t total = pack & 0xFFFFu;
                    for (uint32_t i = (uint32_t)lane * 4u; i < total; i += 4u * WAVE) {
                        const int4 c = ld4(ap4, i >> 2);
                        const uint32_t l0 = (uint32_t)post_doc(c.x, pk) - (uint32_t)base, l1 = (uint32_t)post_doc(c.y, pk) - (uint32_t)base;
                        const uint32_t l2 = (uint32_t)post_doc(c.z, pk) - (uint32_t)base, l3 = (uint32_t)post_doc(c.w, pk) - (uint32_t)base;
                        if (l0 < (uint32_t)R) atomicOr(&sBits[l0 >> 5], 1u << (l0 & 31));
                        if (l1 < (uint32_t)R) atomicOr(&sBits[l1 >> 5], 1u << (l1 & 31));
                        if (l2 < (uint32_t)R) atomicOr(&sBits[l2 >> 5], 1u << (l2 & 31));
                        if (l3 < (uint32_t)R) atomicOr(&sBits[l3 >> 5], 1u << (l3 & 31));
                    }
                } else {
                    const gint32p dp = (gint32p)(uintptr_t)(((unsigned long long)rdl_u(tApHi, tl) << 32) | rdl_u(tApLo, tl)) + mis;
                    for (uint32_t i = lane; i < len; i += WAVE) { int l = post_doc(dp[i], pk) - base; atomicOr(&sBits[l >> 5], 1u << (l & 31)); }
                }
            }
        }
    }
    if (!anyGen) continue;
    if (dbgSkip & 2) continue;
    // lane owns words [lane*WPL, lane*WPL + WPL): contiguous, so slot numbers ascend with the doc id
    uint32_t myBits[WPL]; uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < WPL; j++) { int wi = lane * WPL + j; myBits[j] = wi < W ? sBits[wi] : 0u; cnt += __popc(myBits[j]); }
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) { uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }
    const uint32_t ncand = (uint32_t)rfl_i((int)__shfl(incl, WAVE - 1));      // wave-uniform, and known to be: the group loop of the probe branches on the scalar unit
    if (ncand == 0) continue;
    if ((dbgSkip & 8) && lane == 0) { atomicAdd(&stats[0], 1ull); atomicAdd(&stats[1], (unsigned long long)((ncand + CAP - 1) / CAP)); atomicAdd(&stats[2], (unsigned long long)ncand); }

    // the range's slot block in the query's arena region: ncand slots, filled from the front in doc order
    // (the atomic's return value is first needed when the first round is emitted: its round trip overlaps the term loop)
    uint32_t chunkOffV = 0;
    if (lane == 0) chunkOffV = atomicAdd(&ar.qCursor[q], ncand);
    uint32_t chunkOff = 0; unsigned long long outBase = 0; bool haveOff = false, dropped = false;
    uint32_t written = 0;

    for (uint32_t rb = 0; rb < ncand; rb += (uint32_t)CAP) {
        const uint32_t nslot = min((uint32_t)CAP, ncand - rb);
        const int nGrp = (int)((nslot + WAVE - 1) / WAVE);             // candidate groups in use this round (scalar)
        for (int i = lane * 16; i < R; i += WAVE * 16) *(uint4*)(sTf + i) = make_uint4(0, 0, 0, 0);     // tf array clean at the start of a round
        {                                                      // slot -> doc for this round
            uint32_t sl = incl - cnt;
#pragma unroll
            for (int j = 0; j < WPL; j++) {
                uint32_t bits = myBits[j]; const int wi = lane * WPL + j;
                while (bits) { int bpos = __ffs(bits) - 1; bits &= bits - 1; uint32_t rel = sl - rb; if (rel < nslot) sDoc[rel] = (uint16_t)(wi * 32 + bpos); sl++; }
            }
        }
        // candidate state, one candidate per lane and group
        uint32_t cAddr[G]; float cNorm[G], cAcc[G]; uint32_t cFlag[G], cRank[G], cGrp[G], cExc[G]; unsigned long long cMask[G][MW];
#pragma unroll
        for (int g = 0; g < G; g++) {
            const uint32_t s = (uint32_t)(g * WAVE + lane);
            const bool valid = s < nslot;
            cAddr[g] = valid ? (uint32_t)sDoc[valid ? s : 0] : (uint32_t)(R + 64 + lane);
            cNorm[g] = valid ? ix.docNorm[base + (int)cAddr[g]] : 1.0f;     // one gather per candidate, not per posting
            cAcc[g] = 0.f; cFlag[g] = 0; cRank[g] = 0x1FFu; cGrp[g] = 0; cExc[g] = 0;
#pragma unroll
            for (int w = 0; w < MW; w++) cMask[g][w] = 0ull;
        }
        // ---- 3. every list once, in Bm25Scorer order (ascending termId) ---------------------------------------------------
        // The first 16-byte load of the NEXT non-empty list is issued before the current list is scattered and probed, and inside a
        // list the next 256-posting load is issued before the current one is scattered: most slices are a single load, so without
        // this every list would cost one exposed L2/HBM round trip.
        struct TermS { uint32_t len, total, mis, meta, ref, upd; float idf; gint4p ap; };
        auto read_term = [&](int tl, uint32_t pack, TermS& S) {        // descriptor of the window's term tl, out of the lanes
            S.total = pack & 0xFFFFu; S.mis = (pack >> 16) & 3u; S.ref = (pack >> 18) & 0x1FFFu; S.len = S.total - S.mis;
            S.meta = rdl_u(tMeta, tl); S.upd = rdl_u(tUpd, tl); S.idf = rdl_f(tIdf, tl);
            S.ap = (gint4p)(uintptr_t)(((unsigned long long)rdl_u(tApHi, tl) << 32) | rdl_u(tApLo, tl));
        };
        // probe + BM25+ update of one scattered list, all hit lanes active, no per-hit branches: a lane without a posting reads tf byte 0 and adds nothing
        auto probe = [&](const float idf, const uint32_t upd, const uint32_t ref, const bool unit, const uint32_t grp) {
            const uint32_t addFlag = upd & 0xFFFFu, rk1 = upd >> 16;                          // tier-flag update constants of the term
            const uint32_t capCode = unit ? 1u : 3u;                                           // hit-mask code: 1 (tf 1 / virtual), 2, 3 (tf >= 3)
            const bool wantMask = ar.maskWords != 0 && ref < 32u * (uint32_t)MW;
            const uint32_t sh = (ref & 31u) * 2u;
            const unsigned long long selLo = (MW > 1 && ref >= 32u) ? 0ull : ~0ull;
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (g >= nGrp) break;
                uint32_t tfb = LDS8(cAddr[g]);
                LDS8(cAddr[g]) = 0;                                    // only candidate cells are ever read: the candidate restores its own cell, the
                if (!__ballot(tfb != 0)) continue;                     // cells other postings dirtied are wiped once per round (below), not per list
                if (grp && useGrp) { const bool dup = cGrp[g] == grp; if (tfb) cGrp[g] = grp; if (dup) tfb = 0; }   // union semantics of ExpandMissingTerm (VectorModel.cs:722-731)
                const bool hit = tfb != 0;
                {
                    const float tf = unit ? 1.0f : (float)tfb;        // a virtual term counts every document once (RoaringPostingsEnum.cs:21): member lists scatter the members' real tf bytes
                    const float denom = tf + cNorm[g];
                    const float core = (tf * (1.2f + 1.0f)) / denom;   // (tf * (K1 + 1)) / (tf + normFactor)
                    const float sc = idf * (core + 1.0f);              // idf * (bm25Core + Delta); idf == 0 for a term the scorer skips
                    cAcc[g] += hit ? sc : 0.f;
                }
                cFlag[g] += hit ? addFlag : 0u;                        // AND mode: count of AND-role terms | LOWEST / S1 / S2 bits (each role belongs to one term)
                cRank[g] = min(cRank[g], hit ? rk1 : 0x1FFu);          // disjunctive mode: lowest rank of a generating term that hit
                if (wantMask) {
                    const unsigned long long code = (unsigned long long)min(tfb, capCode) << sh;     // 0 for a lane without a posting
                    if (MW == 2) { cMask[g][0] |= code & selLo; cMask[g][1] |= code & ~selLo; }   // selLo: all ones for reference terms 0..31, else zero (scalar)
                    else if (MW == 1) cMask[g][0] |= code;
                    else {                                                  // four words (a batch with a query of 65 .. 128 reference terms): scalar branch on the word
                        const uint32_t wsel = ref >> 5;
#pragma unroll
                        for (int w = 0; w < MW; w++) if (wsel == (uint32_t)w) cMask[g][w] |= code;
                    }
                    if (!unit && __ballot(tfb >= 3u)) {                // rare: keep the exact tf beside the 2-bit code
                        const uint32_t rec = ((ref + 1u) << 8) | tfb;
                        if (tfb >= 3u) { if (!(cExc[g] & 0xFFFFu)) cExc[g] |= rec; else if (!(cExc[g] >> 16)) cExc[g] |= rec << 16; }
                    }
                }
            }
        };
        // The common visit — a (doc << 8 | tf) index list whose slice fits one 256-posting load, no dedupe group — without the general
        // path's descriptor decoding: two lane reads (idf, tier update) beside the pack word the prefetch already fetched.
        auto fast_list = [&](const int tl, const uint32_t pack, const int4 c) {
            const uint32_t l0 = min(((uint32_t)c.x >> 8) - (uint32_t)base, Rlane), l1 = min(((uint32_t)c.y >> 8) - (uint32_t)base, Rlane);
            const uint32_t l2 = min(((uint32_t)c.z >> 8) - (uint32_t)base, Rlane), l3 = min(((uint32_t)c.w >> 8) - (uint32_t)base, Rlane);
            LDS8(l0) = (uint8_t)c.x; LDS8(l1) = (uint8_t)c.y; LDS8(l2) = (uint8_t)c.z; LDS8(l3) = (uint8_t)c.w;
            probe(rdl_f(tIdf, tl), rdl_u(tUpd, tl), (pack >> 18) & 0x1FFFu, false, 0u);
        };
        auto do_list = [&](const TermS& S, int4 c) {
            const uint32_t iv = (S.meta >> 16) & 0xFFu, grp = S.meta >> 24;
            const bool plain = (iv & 5) != 0 || !ix.packed;            // plain doc ids (host list, device union, unpacked index)
            const bool unit = iv != 0;                                 // virtual term: tf == 1 (RoaringPostingsEnum.cs:21)
            const bool padded = !(iv & 1);                             // index lists and device unions are 16-byte aligned and sentinel padded
            uint32_t l0 = Rlane, l1 = Rlane, l2 = Rlane, l3 = Rlane;
            if (!plain) {
                // (doc << 8) | tf words: ds_write_b8 stores the low byte = tf.  Lists are 16-byte aligned and sentinel padded, so elements outside
                // the slice are same-list postings of other ranges or sentinels: the range check alone routes them to the dummy zone.
                // The first (usually only) 256-posting load arrived through the prefetch: scattered straight from its registers; only a
                // longer slice enters the loop (its own one-ahead prefetch), so the common visit carries no loop state (register copies).
                l0 = min(((uint32_t)c.x >> 8) - (uint32_t)base, Rlane); l1 = min(((uint32_t)c.y >> 8) - (uint32_t)base, Rlane);
                l2 = min(((uint32_t)c.z >> 8) - (uint32_t)base, Rlane); l3 = min(((uint32_t)c.w >> 8) - (uint32_t)base, Rlane);
                LDS8(l0) = (uint8_t)c.x; LDS8(l1) = (uint8_t)c.y; LDS8(l2) = (uint8_t)c.z; LDS8(l3) = (uint8_t)c.w;
                if (S.total > 4u * WAVE) {
                    const uint32_t li = (uint32_t)lane * 4u;
                    int4 cur = make_int4(-1, -1, -1, -1);
                    if (4u * WAVE + li < S.total) cur = ld4(S.ap, (4u * WAVE + li) >> 2);
                    for (uint32_t off = 4 * WAVE; off < S.total; off += 4 * WAVE) {
                        int4 nxt = make_int4(-1, -1, -1, -1);
                        const uint32_t nidx = off + 4 * WAVE + li;
                        if (nidx < S.total) nxt = ld4(S.ap, nidx >> 2);
                        const uint32_t m0 = min(((uint32_t)cur.x >> 8) - (uint32_t)base, Rlane), m1 = min(((uint32_t)cur.y >> 8) - (uint32_t)base, Rlane);
                        const uint32_t m2 = min(((uint32_t)cur.z >> 8) - (uint32_t)base, Rlane), m3 = min(((uint32_t)cur.w >> 8) - (uint32_t)base, Rlane);
                        LDS8(m0) = (uint8_t)cur.x; LDS8(m1) = (uint8_t)cur.y; LDS8(m2) = (uint8_t)cur.z; LDS8(m3) = (uint8_t)cur.w;
                        cur = nxt;
                    }
                }
            } else {
                // plain doc ids (host list, device union, unpacked index): padded lists as above; host-supplied lists keep the index check
                uint32_t mis = S.mis; asm volatile("" : "+s"(mis));     // keeps this path's address arithmetic out of the common path
                const uint8_t* wp = unit ? nullptr : ix.postW + ((const int32_t*)(uintptr_t)S.ap + mis - ix.postDoc);     // unpacked index lists live in postDoc
                for (uint32_t off = 0; off < S.total; off += 4 * WAVE) {
                    const uint32_t idx = off + (uint32_t)lane * 4u;
                    int4 nxt = make_int4(-1, -1, -1, -1);
                    const uint32_t nidx = idx + 4 * WAVE;
                    if (nidx < S.total) nxt = ld4(S.ap, nidx >> 2);
                    const uint32_t rel0 = idx - mis;                   // posting number of element 0 (wraps below 0 before the slice)
                    const bool v0 = padded || rel0 < S.len, v1 = padded || rel0 + 1u < S.len, v2 = padded || rel0 + 2u < S.len, v3 = padded || rel0 + 3u < S.len;
                    l0 = v0 ? min((uint32_t)c.x - (uint32_t)base, Rlane) : Rlane; l1 = v1 ? min((uint32_t)c.y - (uint32_t)base, Rlane) : Rlane;
                    l2 = v2 ? min((uint32_t)c.z - (uint32_t)base, Rlane) : Rlane; l3 = v3 ? min((uint32_t)c.w - (uint32_t)base, Rlane) : Rlane;
                    uint8_t t0 = 1, t1 = 1, t2 = 1, t3 = 1;
                    if (!unit) {                                       // unpacked index (shards of >= 2^24 - R documents): tf from the byte array
                        t0 = l0 < (uint32_t)R ? wp[rel0] : 1; t1 = l1 < (uint32_t)R ? wp[rel0 + 1u] : 1; t2 = l2 < (uint32_t)R ? wp[rel0 + 2u] : 1; t3 = l3 < (uint32_t)R ? wp[rel0 + 3u] : 1;
                    }
                    LDS8(l0) = t0; LDS8(l1) = t1; LDS8(l2) = t2; LDS8(l3) = t3;
                    c = nxt;
                }
            }
            probe(S.idf, S.upd, S.ref, unit, grp);
        };
        // The first 16-byte load of the next non-empty lists is issued before the current list is scattered and probed (most slices are a
        // single load: without this every list costs one exposed L2/HBM round trip).  Measured alternatives on the 10 M-doc batch: batches
        // of six loads selected by a switch (12.1 ms, 152 VGPRs) and the same under a 128-VGPR cap (11.5 ms, scratch spills) lose to this
        // rotating window (9.2 ms): occupancy matters more than prefetch depth here.  Round 3: an unrolled ring of three or four UNCONDITIONAL loads (no register
        // copies, so the compiler waits with vmcnt(2) instead of draining the queue at every visit) spills at this kernel's 128-VGPR budget: 7.73 vs 7.40 ms.
        if (!(dbgSkip & 1)) for (int win = 0; win < nWin; win++) {
            if (nWin > 1) { load_window_consts(win); locate_window(r, base, rend); }
            unsigned long long tmask = __ballot(tLen > 0);             // the window's non-empty slices, ascending term order
            if (!tmask) continue;
            auto next_tl = [&]() -> int { if (!tmask) return -1; const int t = __ffsll((long long)tmask) - 1; tmask &= tmask - 1; return t; };
            auto issue = [&](int tl, uint32_t& pack) -> int4 {
                int4 c = make_int4(-1, -1, -1, -1); pack = 0;
                if (tl >= 0) {
                    pack = rdl_u(tPack, tl);
                    const gint4p ap = (gint4p)(uintptr_t)(((unsigned long long)rdl_u(tApHi, tl) << 32) | rdl_u(tApLo, tl));
                    if ((uint32_t)lane * 4u < (pack & 0xFFFFu)) c = ld4(ap, (uint32_t)lane);
                }
                return c;
            };
            uint32_t p0, p1, p2;
            int t0 = next_tl(); int4 c0 = issue(t0, p0);
            int t1 = next_tl(); int4 c1 = issue(t1, p1);
            while (t0 >= 0) {
                const int t2 = next_tl(); const int4 c2 = issue(t2, p2);
                if (p0 >> 31) fast_list(t0, p0, c0);
                else { TermS A; read_term(t0, p0, A); do_list(A, c0); }
                t0 = t1; c0 = c1; p0 = p1; t1 = t2; c1 = c2; p1 = p2;
            }
        }
        if (dbgSkip & 4) continue;
        // ---- 4. classify + count + compact ---------------------------------------------------------------------------------
        if (!haveOff) {
            chunkOff = (uint32_t)rfl_i((int)chunkOffV); haveOff = true;
            if (chunkOff + ncand > qcap) { if (lane == 0) atomicExch(ar.overflow, 1u); dropped = true; }
            outBase = qb + chunkOff;
        }
        if (dropped) break;
#pragma unroll
        for (int g = 0; g < G; g++) {
            if ((uint32_t)(g * WAVE) >= nslot) break;
            const uint32_t s = (uint32_t)(g * WAVE + lane);
            bool emit = false; uint8_t cls = 0; const float sc = cAcc[g]; const uint32_t f = (mode == INFX_MODE_DISJ) ? (cRank[g] == 0x1FFu ? 0u : cRank[g]) : cFlag[g]; const int l = (int)cAddr[g];
            if (s < nslot && sc > 0.f) {
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
                            int32_t d = base + l;
                            uint64_t p = lower_bound_i32(ix.psDocs, psBase, psBase + psLen, d);
                            pre = p < psBase + psLen && ix.psDocs[p] == d;
                        }
                        if (pre) cls |= 0x80; else atomicAdd(&sHist[cls], 1u);
                    }
                } else { emit = true; cls = 1; atomicAdd(&sHist[1], 1u); }
            }
            const unsigned long long m = __ballot(emit);
            if (emit) {
                const unsigned long long pos = outBase + written + __popcll(m & ((1ull << lane) - 1));
                ar.doc[pos] = ix.docBase + base + l;
                // Document.Deleted (Bm25Scorer.cs:322-323): the row stays (tier counts and the reference's chunk positions include it) with score 0 —
                // k_select and the replay's heap never see it.  One byte gather per emitted row, only while the index holds deletions.
                const float stored = (del && del[ix.docBase + base + l]) ? 0.f : sc;
                ar.score[pos] = stored; myMax = max(myMax, __float_as_uint(stored));
                ar.cls[pos] = cls;
                if (ar.maskWords) {
#pragma unroll
                    for (int w = 0; w < MW; w++) ar.mask[pos * (unsigned long long)MW + w] = cMask[g][w];
                    ar.exc[pos] = cExc[g];
                }
            }
            written += (uint32_t)__popcll(m);
        }
    }
    // directory entry + holes (slots of candidates that were not emitted)
    if (!haveOff || dropped) continue;
    if (lane == 0) { ar.dir[(unsigned long long)q * ix.nRanges + r] = make_uint2(chunkOff, written); myBytes += (unsigned long long)written * 12ull; }
    for (uint32_t i = written + lane; i < ncand; i += WAVE) { ar.cls[outBase + i] = CLS_HOLE; ar.score[outBase + i] = 0.f; }     // k_select skips rows with score bits 0
    }   // ranges of the stripe
    for (int i = lane; i < INFX_NCLASS; i += WAVE) { uint32_t c = sHist[i]; if (c) atomicAdd(&ar.counts[(uint64_t)q * INFX_NCLASS + i], c); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) myBytes += __shfl_down(myBytes, d);
    if (lane == 0 && myBytes) atomicAdd(&ar.qBytes[q], myBytes);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) myMax = max(myMax, (uint32_t)__shfl_down((int)myMax, d));
    if (lane == 0 && myMax) atomicMax(&ar.qMax[q], myMax);
}

// k_union — fuzzy virtual terms (ExpandMissingTerm, VectorModel.cs:643-743) on the device: the union of the member terms' doc sets
// of this shard.  One wave per (virtual term, doc range): member slices OR-ed into an LDS bitmap.
//   pass 0 (outDocs == nullptr): rangeCount[v][r] = popcount           -> k_union_scan: per-term exclusive scan + total (= shard df)
//   pass 1: the range's documents are written, ascending, at outDocs[unionBase[v] + rangeCount[v][r]] (rangeCount now holds offsets)
template <int R>
__global__ __launch_bounds__(WAVE) void k_union(DevIndex ix, const uint32_t* __restrict__ memberBeg, const uint32_t* __restrict__ memberEnd, const int32_t* __restrict__ members,
                                                 uint32_t nv, uint32_t* __restrict__ rangeCount, const unsigned long long* __restrict__ unionBase,
                                                 int32_t* __restrict__ outDocs) {
    constexpr int W = R / 32;
    constexpr int WPL = (W + WAVE - 1) / WAVE;
    __shared__ uint32_t sBits[W];
    __shared__ unsigned long long sBase[WAVE];
    __shared__ uint32_t sLen[WAVE];
    const int lane = threadIdx.x;
    const uint32_t v = blockIdx.x % nv; const int r = (int)(blockIdx.x / nv);
    const int32_t base = r * R, rend = min(base + R, ix.N);
    if (outDocs) { if (r + 1 <= ix.nRanges && rangeCount[(uint64_t)v * (ix.nRanges + 1) + r] == rangeCount[(uint64_t)v * (ix.nRanges + 1) + r + 1]) return; }   // empty range
    for (int i = lane; i < W; i += WAVE) sBits[i] = 0;
    const uint32_t mb = memberBeg[v], me = memberEnd[v];      // (a CSR caller passes offs and offs + 1; the fused LD1 path passes ranges k_ld1 closed on the device)
    bool any = false;
    for (uint32_t m0 = mb; m0 < me; m0 += WAVE) {
        uint32_t len = 0; unsigned long long b0 = 0;
        if (m0 + lane < me) {
            const int32_t t = members[m0 + lane];
            const uint64_t tb = ix.postOff[t], te = ix.postOff[t + 1];
            const uint32_t sk = ix.skipIdx[t];
            uint32_t lo, hi;
            if (sk != 0xFFFFFFFFu) { lo = ix.skipTbl[sk + r]; hi = ix.skipTbl[sk + r + 1]; }
            else { lo = (uint32_t)(lower_bound_post(ix.postDoc, tb, te, base, ix.packed) - tb); hi = (uint32_t)(lower_bound_post(ix.postDoc, tb + lo, te, rend, ix.packed) - tb); }
            len = hi - lo; b0 = tb + lo;
        }
        sBase[lane] = b0; sLen[lane] = len;
        const int nm = (int)min((uint32_t)WAVE, me - m0);
        for (int k = 0; k < nm; k++) {
            const uint32_t L = sLen[k]; const unsigned long long bb = sBase[k];
            if (L) any = true;
            for (uint32_t i = lane; i < L; i += WAVE) { int l = post_doc(ix.postDoc[bb + i], ix.packed) - base; atomicOr(&sBits[l >> 5], 1u << (l & 31)); }
        }
    }
    if (!outDocs) {
        uint32_t c = 0;
        if (any) for (int i = lane; i < W; i += WAVE) c += __popc(sBits[i]);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
        if (lane == 0) rangeCount[(uint64_t)v * (ix.nRanges + 1) + r] = c;
        return;
    }
    if (!any) return;
    // lane owns words [lane*WPL, lane*WPL+WPL): ascending doc order
    uint32_t myBits[WPL]; uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < WPL; j++) { int wi = lane * WPL + j; myBits[j] = wi < W ? sBits[wi] : 0u; cnt += __popc(myBits[j]); }
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) { uint32_t x = __shfl_up(incl, d); if (lane >= d) incl += x; }
    unsigned long long o = unionBase[v] + rangeCount[(uint64_t)v * (ix.nRanges + 1) + r] + (incl - cnt);
#pragma unroll
    for (int j = 0; j < WPL; j++) {
        uint32_t bits = myBits[j]; const int wi = lane * WPL + j;
        while (bits) { int bpos = __ffs(bits) - 1; bits &= bits - 1; outDocs[o++] = base + wi * 32 + bpos; }
    }
}
// per virtual term: exclusive scan of its nRanges counts in place (entry nRanges = total)
__global__ __launch_bounds__(256) void k_union_scan(uint32_t* __restrict__ rangeCount, int nRanges, uint32_t* __restrict__ totals) {
    __shared__ uint32_t sPart[256];
    const uint32_t v = blockIdx.x; const int tid = threadIdx.x;
    uint32_t* rc = rangeCount + (uint64_t)v * (nRanges + 1);
    const int per = (nRanges + 255) / 256;
    const int b0 = tid * per, b1 = min(nRanges, b0 + per);
    uint32_t s = 0; for (int i = b0; i < b1; i++) s += rc[i];
    sPart[tid] = s; __syncthreads();
    if (tid == 0) { uint32_t run = 0; for (int i = 0; i < 256; i++) { uint32_t x = sPart[i]; sPart[i] = run; run += x; } totals[v] = run; rc[nRanges] = run; }
    __syncthreads();
    uint32_t run = sPart[tid];
    for (int i = b0; i < b1; i++) { uint32_t x = rc[i]; rc[i] = run; run += x; }
}

// ---------------------------------------------------------------------------------------------------------------
// k_select: one 1024-thread workgroup per query. Radix select (12-bit digits) on the 64-bit composite key
//   (score bits << 32) | (0xFFFFFFFF - doc)   — descending — over the query's contiguous arena region,
// then an LDS bitonic sort of the <= SEL_CAP survivors.  Replaces UpdateTopK / PriorityQueue (Bm25Scorer.cs:654-670).
#define SEL_THREADS 1024
#define SEL_WAVES (SEL_THREADS / WAVE)
#define SEL_CAP 2048      // survivors sorted in LDS (>= 2 * max depth)
#define SEL_AMBIG_REL 1e-5f   // >> the few-ulp (measured <= 2.8e-7 relative) score differences the reference's two BM25 formulations can cause

__device__ __forceinline__ bool sel_pass(const SelRule& rule, uint8_t c) {
    if (rule.mode == INFX_MODE_AND) return (c & rule.classMask) != 0;
    if (rule.mode == INFX_MODE_DISJ) return (int)(c & 0x7F) <= rule.cutoffRank;
    return true;
}
__device__ __forceinline__ unsigned long long sel_key(const Arena& ar, uint64_t i) {
    return ((unsigned long long)__float_as_uint(ar.score[i]) << 32) | (0xFFFFFFFFu - (uint32_t)ar.doc[i]);
}

// One sweep over a query's arena rows: SEL_U rows per thread and trip, class byte and score of all of them loaded as independent requests (a hole or a
// row the rule rejects costs its 4 score bytes; the dependent class -> score chain it replaces doubled the latency of every trip, and the kernel's time
// is the latency chain of its largest queries).  f(score bits, row index) is called for the rows that pass the rule and hold a positive score.
#ifndef SEL_U
#define SEL_U 8
#endif
template <class F> __device__ __forceinline__ void sel_sweep(const Arena& ar, const SelRule& rule, uint64_t qb, uint32_t qn, int tid, F&& f) {
    for (uint32_t i0 = tid; i0 < qn; i0 += SEL_U * SEL_THREADS) {
        uint8_t c[SEL_U]; uint32_t sb[SEL_U];
#pragma unroll
        for (int u = 0; u < SEL_U; u++) { const uint32_t i = i0 + u * SEL_THREADS; c[u] = i < qn ? ar.cls[qb + i] : (uint8_t)CLS_HOLE; sb[u] = i < qn ? __float_as_uint(ar.score[qb + i]) : 0u; }
#pragma unroll
        for (int u = 0; u < SEL_U; u++) if (sb[u] && sel_pass(rule, c[u])) f(sb[u], i0 + u * SEL_THREADS);      // holes and deleted documents carry score bits 0
    }
}

// Longest queries first: k_select runs one workgroup per query and its duration is the tail of the few queries with 10^5 .. 10^6 rows (a 1000-query batch at
// 10 M documents: median 13 k rows, maximum 1.6 M).  Workgroups start in blockIdx order, so the batch's queries are ordered by their row count, descending
// (one workgroup, LDS bitonic sort of <= SEL_ORDER_MAX keys), and k_select's block b takes query order[b]: the giants start in the first wave of workgroups
// instead of wherever their query number puts them.
#define SEL_ORDER_MAX 4096
__global__ __launch_bounds__(1024) void k_select_order(const uint32_t* __restrict__ qCursor, uint32_t nq, uint32_t* __restrict__ order) {
    __shared__ unsigned long long sK[SEL_ORDER_MAX];
    const uint32_t tid = threadIdx.x;
    uint32_t m = 2; while (m < nq) m <<= 1;
    for (uint32_t i = tid; i < m; i += 1024) sK[i] = i < nq ? (((unsigned long long)qCursor[i] << 32) | (0xFFFFFFFFu - i)) : 0ull;      // ties: lower query first
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (m >> 1); t += 1024) {
                const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const unsigned long long va = sK[a], vb = sK[b];
                const bool desc = (a & k) == 0;
                if (desc ? (va < vb) : (va > vb)) { sK[a] = vb; sK[b] = va; }
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < nq; i += 1024) order[i] = 0xFFFFFFFFu - (uint32_t)sK[i];
}
// ---- the batch's largest queries: histogram and gather sweeps spread over many workgroups (round 6) ---------------------------------------------------------
// k_select runs one workgroup per query, and one workgroup streams ~20-30 GB/s (a CU's share of HBM, whatever it keeps in flight): the 1.7 M rows of a batch's largest
// query took 1.0 ms (0.41 histogram sweep + 0.58 gather sweep) while 99 % of the batch's workgroups had ended after 0.45 ms — k_select's duration was that tail
// (per-workgroup timestamps, profiles/r06_select_giants.md).  The first SELG_MAX queries of the longest-first order that hold >= minRows rows are swept by up to
// SELG_PARTS workgroups each, in launches in front of k_select:
//   k_selg_hist    every partition's histograms (k_select's 4095 bins of 2^12 score bits below the query's best row, and 4095 bins of 2^16) added into global ones;
//   k_selg_cut     one workgroup per query: the cut bin (k_select's find_bin) in the fine histogram, else the coarse one, and whether the rows down to that bin fit
//                  the LDS sort (k_select's "mode 1"); a query with no more rows passing its rule than the sort holds takes all of them;
//   k_selg_gather  every partition appends its rows down to the cut bin to the query's key list (collected in LDS, one global atomic per partition: one per row
//                  serialised at L2 and cost 0.4 ms) and keeps the best row left out.
// k_select then starts at its sort for such a query; any other case (an exact plateau wider than the sort across the cut, the window missed twice) leaves mode 0 and
// k_select does all the work itself, as before.  The key list holds every row at or above the cut bin's lower edge, a superset of the top `depth` whatever the bin
// width or origin: same rows after the sort, same best row left out: bit-identical (tests/test_gpu_select_cuts.py holds every path of the cut — swept fine, coarse,
// take-all and refused among them — to the plain model tests/select_model.py row for row, under INFX_SEL_GIANT_MIN = 64, 16384 and 0;
// tests/test_gpu_parity.py::test_accumulate_schedules_agree_bit_for_bit runs INFX_SEL_GIANT_MIN = 64 and 3000 against 0; tests/test_gpu_fullsize.py runs the default at
// 10 M documents against the oracle).
// Per 1000-query launch at 10 M documents: k_select 1.06 ms -> 0.18 + 0.11 (hist) + 0.03 (cut) + 0.14 (gather) = 0.46 ms.
#define SELG_MAX 256
#define SELG_SHIFT2 16                     // bin width (score bits) of the coarse histogram: a window of 2^28 below the best row
#define SELG_PARTS 32
#define SELG_PART_MIN 16384
struct SelGiant { uint32_t* hist; uint32_t* count; uint32_t* left; uint32_t* mode; uint32_t* cut; uint32_t* shift; unsigned long long* keys; uint32_t minRows; };
__device__ __forceinline__ bool selg_part(const Arena& ar, const SelRule* __restrict__ rules, const uint32_t* __restrict__ order, uint32_t nq, const SelGiant& G,
                                          int& q, uint64_t& qb, uint32_t& r0, uint32_t& rn) {
    const uint32_t g = blockIdx.y, p = blockIdx.x;
    if (g >= nq) return false;
    q = (int)order[g];
    const uint32_t qn = ar.qCursor[q];
    if (qn < G.minRows) return false;
    const uint32_t per = max((uint32_t)SELG_PART_MIN, (qn + SELG_PARTS - 1) / SELG_PARTS);
    r0 = p * per;
    if (r0 >= qn) return false;
    rn = min(qn - r0, per); qb = ar.qBase[q] + r0;
    return true;
}
__global__ __launch_bounds__(SEL_THREADS) void k_selg_hist(Arena ar, const SelRule* __restrict__ rules, const uint32_t* __restrict__ order, uint32_t nq, SelGiant G) {
    __shared__ uint32_t hist[2 * 4096];      // [0, 4096): k_select's bins, 2^12 score bits wide (the top rows within a factor 4 of the best); [4096, 8192): 2^16 wide, for a query whose
                                             // top rows spread further or lie far below the best row of a class the rule rejects (k_select sweeps for the best PASSING row then: three sweeps)
    int q; uint64_t qb; uint32_t r0, rn; const int tid = threadIdx.x;
    if (!selg_part(ar, rules, order, nq, G, q, qb, r0, rn)) return;
    const SelRule rule = rules[q];
    const uint32_t M = ar.qMax[q];              // the histograms' origin: the best score of ALL the query's rows (k_accumulate leaves it), >= every row the rule lets through
    if (!M || rule.total <= (uint32_t)SEL_CAP) return;      // (few enough rows pass the rule: all of them are taken, no histogram)
    for (uint32_t i = tid; i < 2 * 4096; i += SEL_THREADS) hist[i] = 0;
    __syncthreads();
    sel_sweep(ar, rule, qb, rn, tid, [&](uint32_t sb, uint32_t) {
        const uint32_t d = M - sb, b = d >> 12, b2 = d >> SELG_SHIFT2;
        if (b < 4095u) atomicAdd(&hist[b], 1u);
        if (b2 < 4095u) atomicAdd(&hist[4096 + b2], 1u);
    });
    __syncthreads();
    for (uint32_t i = tid; i < 2 * 4096; i += SEL_THREADS) { const uint32_t c = hist[i]; if (c) atomicAdd(&G.hist[(size_t)blockIdx.y * 2 * 4096 + i], c); }
}
// the cut bin of every swept query, once (k_select's find_bin over the global histogram); mode 1 = "the rows down to the cut bin fit the LDS sort" (k_select's own mode 1)
__global__ __launch_bounds__(256) void k_selg_cut(Arena ar, const SelRule* __restrict__ rules, const uint32_t* __restrict__ order, uint32_t nq, SelGiant G) {
    __shared__ uint32_t hist[4096];
    __shared__ uint32_t part[256];
    __shared__ uint32_t sOk;
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    if (g >= nq) return;
    const int q = (int)order[g];
    if (ar.qCursor[q] < G.minRows) return;
    if (rules[q].total <= (uint32_t)SEL_CAP) { if (tid == 0) { G.cut[g] = 0xFFFFFFFFu; G.shift[g] = 12u; G.mode[g] = 1u; } return; }      // take every row the rule lets through (k_select's general path does)
    if (!ar.qMax[q]) return;
    const uint32_t want = (uint32_t)rules[q].depth;
    for (int level = 0; level < 2; level++) {                                // the fine histogram first (what k_select itself would use), the coarse one if its window misses the cut
        __syncthreads();
        for (uint32_t i = tid; i < 4096; i += 256) hist[i] = i < 4095u ? G.hist[((size_t)g * 2 + level) * 4096 + i] : 0u;
        __syncthreads();
        { uint32_t c = 0; for (uint32_t j = 0; j < 16; j++) c += hist[tid * 16 + j]; part[tid] = c; }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0, c = 0;
            for (; c < 256u; c++) { if (acc + part[c] >= want) break; acc += part[c]; }
            uint32_t bsel = 4096;
            if (c < 256u) for (uint32_t j = 0; j < 16; j++) { const uint32_t bin = c * 16 + j; if (acc + hist[bin] >= want) { bsel = bin; break; } acc += hist[bin]; }
            // (bsel == 4096: fewer rows inside the window than the depth — whether rows lie beyond it is unknown here)
            const uint32_t above1 = acc, und1 = bsel < 4096u ? hist[bsel] : 0u;
            sOk = (bsel < 4095u && above1 + und1 <= (uint32_t)SEL_CAP) ? 1u : 0u;
            if (sOk) { G.cut[g] = bsel; G.shift[g] = level ? SELG_SHIFT2 : 12u; G.mode[g] = 1u; }
        }
        __syncthreads();
        if (sOk) break;
    }
}
__global__ __launch_bounds__(SEL_THREADS) void k_selg_gather(Arena ar, const SelRule* __restrict__ rules, const uint32_t* __restrict__ order, uint32_t nq, SelGiant G) {
    __shared__ unsigned long long lk[SEL_CAP];
    __shared__ uint32_t lCount, lBase;
    int q; uint64_t qb; uint32_t r0, rn; const int tid = threadIdx.x;
    if (!selg_part(ar, rules, order, nq, G, q, qb, r0, rn)) return;
    const uint32_t g = blockIdx.y;
    if (G.mode[g] != 1u) return;                                             // not k_select's mode 1 (or no row passes): k_select does this query itself
    const uint32_t M = ar.qMax[q], b1 = G.cut[g], sh = G.shift[g];          // (take-all: b1 = ~0 — every row compares below)
    const SelRule rule = rules[q];
    __shared__ uint32_t sLm;
    if (tid == 0) { lCount = 0; sLm = 0; }
    __syncthreads();
    uint32_t leftMax = 0;
    sel_sweep(ar, rule, qb, rn, tid, [&](uint32_t sb, uint32_t i) {
        if (((M - sb) >> sh) <= b1) lk[atomicAdd(&lCount, 1u)] = ((unsigned long long)sb << 32) | (0xFFFFFFFFu - (uint32_t)ar.doc[qb + i]);      // (all partitions together hold <= SEL_CAP such rows)
        else leftMax = max(leftMax, sb);
    });
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) leftMax = max(leftMax, (uint32_t)__shfl_xor((int)leftMax, d));
    if ((tid & 63) == 0 && leftMax) atomicMax(&sLm, leftMax);
    __syncthreads();
    if (tid == 0) { lBase = lCount ? atomicAdd(&G.count[g], lCount) : 0u; if (sLm) atomicMax(&G.left[g], sLm); }      // one global atomic each per partition (one per row serialised at L2: 0.4 ms)
    __syncthreads();
    for (uint32_t i = tid; i < lCount; i += SEL_THREADS) if (lBase + i < (uint32_t)SEL_CAP) G.keys[(size_t)g * SEL_CAP + lBase + i] = lk[i];
}

#ifdef SEL_PROF
__device__ unsigned long long* g_selProf = nullptr;
#define SELP(i) do { if (g_selProf && tid == 0) g_selProf[(size_t)q * 8 + (i)] = wall_clock64(); } while (0)
#else
#define SELP(i)
#endif
__global__ __launch_bounds__(SEL_THREADS) void k_select(Arena ar, int nRanges, const SelRule* __restrict__ rules,
                                                         infx_hit* __restrict__ out, uint32_t* __restrict__ outCount, int outStride, uint32_t* __restrict__ flagged,
                                                         uint32_t* __restrict__ flagStats, float* __restrict__ nextOut, const uint32_t* __restrict__ order, SelGiant G) {
    __shared__ uint32_t hist[4096];
    __shared__ uint32_t part[256];
    __shared__ unsigned long long keys[SEL_CAP];
    __shared__ uint32_t sCount, sBin, sRemain, sLeft;
    __shared__ uint32_t sMax[SEL_WAVES];
    const int q = order ? (int)order[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const SelRule rule = rules[q];
    const int depth = rule.depth;
    const uint64_t qb = ar.qBase[q];
    const uint32_t qn = ar.qCursor[q];          // entries of this query: arena[qb, qb+qn), contiguous
    if (tid == 0) { sCount = 0; sLeft = 0; sRemain = 0; }
    uint32_t leftMax = 0;                       // best score (bits) among the rows this thread saw and did NOT gather
    SELP(0);
#ifdef SEL_PROF
    if (g_selProf && tid == 0) { g_selProf[(size_t)q * 8 + 6] = qn; g_selProf[(size_t)q * 8 + 1] = 0; g_selProf[(size_t)q * 8 + 2] = 0; }
#endif

    // ---- fast path (round 4): the top-`depth` rows lie within a factor 4 of the query's best score for all but a few queries, so ONE histogram pass over
    // 4095 bins LINEAR in the score bits below the maximum (2^12 ulps wide) isolates them; a second pass over the 12 low bits decides the score exactly.
    // (The bit-field radix below spends its first pass on the sign / exponent / top mantissa bits, which all rows of a query share.)  Rows further below
    // the maximum are not counted.  An exact score plateau across the cut that does not fit the LDS sort is NOT cut by doc id when the exact replay
    // follows (flagged != nullptr): the replay overrides this kernel's list for every flagged query, so the remaining radix passes would be wasted.
    bool gathered = false;
    if (G.mode && order && blockIdx.x < SELG_MAX && G.mode[blockIdx.x] == 1u) {      // swept by k_selg_hist / k_selg_gather: the keys are waiting
        const uint32_t n = min(G.count[blockIdx.x], (uint32_t)SEL_CAP);
        for (uint32_t i = tid; i < n; i += SEL_THREADS) keys[i] = G.keys[(size_t)blockIdx.x * SEL_CAP + i];
        if (tid == 0) { sCount = n; sLeft = G.left[blockIdx.x]; }
        gathered = true;
    } else
    if (rule.total > (uint32_t)SEL_CAP) {       // (a query with fewer rows than the sort holds is gathered whole by the general path)
        // The histogram's origin M only has to be >= every row the rule lets through.  Round 5: k_accumulate leaves the best score of ALL the query's rows in
        // qMax (one atomicMax per wave), so the sweep that used to find the maximum of the passing rows is skipped; if the top-`depth` passing rows lie outside
        // the window below that origin (rows of a rejected class score far above them: rare) the sweep runs after all and the histogram is taken again.
        uint32_t M = ar.qMax[q];
        auto find_bin = [&](uint32_t nb, uint32_t want) {
            const uint32_t per = nb / 256;
            if ((uint32_t)tid < 256u) { uint32_t c = 0; for (uint32_t j = 0; j < per; j++) c += hist[(uint32_t)tid * per + j]; part[tid] = c; }
            __syncthreads();
            if (tid == 0) {
                uint32_t acc = 0, c = 0;
                for (; c < 256u; c++) { if (acc + part[c] >= want) break; acc += part[c]; }
                uint32_t bsel = nb;
                if (c < 256u) for (uint32_t j = 0; j < per; j++) { const uint32_t bin = c * per + j; if (acc + hist[bin] >= want) { bsel = bin; break; } acc += hist[bin]; }
                sBin = bsel; sRemain = want - acc; sCount = bsel < nb ? hist[bsel] : 0u;
            }
            __syncthreads();
        };
        for (int attempt = M ? 0 : 1; attempt < 2; attempt++) {      // (M == 0: an accumulation kernel that does not keep the maximum — the A/B designs of the experiments build)
            if (attempt == 1) {
                uint32_t mx = 0;
                sel_sweep(ar, rule, qb, qn, tid, [&](uint32_t sb, uint32_t) { mx = max(mx, sb); });
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
                __syncthreads();
                if ((tid & 63) == 0) sMax[tid >> 6] = mx;
                __syncthreads();
                M = 0;
#pragma unroll
                for (int w = 0; w < SEL_WAVES; w++) M = max(M, sMax[w]);
            }
            for (uint32_t i = tid; i < 4096; i += SEL_THREADS) hist[i] = 0;
            __syncthreads();
            sel_sweep(ar, rule, qb, qn, tid, [&](uint32_t sb, uint32_t) { const uint32_t b = (M - sb) >> 12; if (b < 4095u) atomicAdd(&hist[b], 1u); });
            __syncthreads();
            find_bin(4096u, (uint32_t)depth);           // bin 4095 is never counted: reaching it means "outside the fast path's range"
            if (sBin < 4095u || attempt == 1) break;
            __syncthreads();
        }
        // (find_bin: first bin — ascending = descending score — at which the running count reaches `want`: sBin = bin (nb: never), sRemain = want - rows before it,
        //  sCount = rows in it)
        const uint32_t b1 = sBin, rem1 = sRemain, und1 = sCount;
        __syncthreads();
        SELP(1);
        int mode = 0; uint32_t b2 = 0, takeAbove = 0;      // 1: rows with bin <= b1; 2: bin < b1, or bin == b1 and low bits <= b2; 3: as 2 with the plateau capped
        if (b1 < 4095u) {
            const uint32_t above1 = (uint32_t)depth - rem1;
            if (above1 + und1 <= (uint32_t)SEL_CAP) mode = 1;
            else {
                for (uint32_t i = tid; i < 4096; i += SEL_THREADS) hist[i] = 0;
                __syncthreads();
                sel_sweep(ar, rule, qb, qn, tid, [&](uint32_t sb, uint32_t) { const uint32_t d = M - sb; if ((d >> 12) == b1) atomicAdd(&hist[d & 4095u], 1u); });
                __syncthreads();
                find_bin(4096u, rem1);
                b2 = sBin;
                const uint32_t rem2 = sRemain, und2 = sCount;
                __syncthreads();
                takeAbove = above1 + (rem1 - rem2);           // rows strictly better than the score at the cut
                if (b2 < 4096u) {
                    if (takeAbove + und2 <= (uint32_t)SEL_CAP) mode = 2;
                    else if (flagged) mode = 3;               // exact plateau across the cut, larger than the sort: the replay decides it
                }
            }
        }
        SELP(2);
        if (mode) {
            if (tid == 0) { sCount = 0; sRemain = 0; }
            __syncthreads();
            const uint32_t platCap = (uint32_t)SEL_CAP - takeAbove;          // mode 3: plateau rows admitted
            sel_sweep(ar, rule, qb, qn, tid, [&](uint32_t sb, uint32_t i) {
                const uint32_t dlt = M - sb, bn = dlt >> 12, lo = dlt & 4095u;
                bool take;
                if (mode == 1) take = bn <= b1;
                else {
                    take = bn < b1 || (bn == b1 && lo <= b2);
                    if (take && mode == 3 && bn == b1 && lo == b2) take = atomicAdd(&sRemain, 1u) < platCap;
                }
                if (take) {
                    const unsigned long long k = ((unsigned long long)sb << 32) | (0xFFFFFFFFu - (uint32_t)ar.doc[qb + i]);
                    const uint32_t q2 = atomicAdd(&sCount, 1u); if (q2 < SEL_CAP) keys[q2] = k;
                } else leftMax = max(leftMax, sb);
            });
            gathered = true;
        }
    }

    if (!gathered) {
    unsigned long long prefix = 0, mask = 0;   // keys with (key & mask) == prefix are "undecided"
    uint32_t remain = (uint32_t)depth;         // how many still to take from the undecided set
    uint32_t undecided = rule.total;           // upper bound on the filtered entries of this query
    int shift = 52, width = 12;
    while ((uint32_t)depth - remain + undecided > (uint32_t)SEL_CAP && shift >= 0) {
        const uint32_t nb = 1u << width, dm = nb - 1u;
        for (uint32_t i = tid; i < nb; i += SEL_THREADS) hist[i] = 0;
        __syncthreads();
        if (shift >= 32) {                 // digit and decided prefix lie inside the score bits: the doc ids are not read in this pass
            sel_sweep(ar, rule, qb, qn, tid, [&](uint32_t sb, uint32_t) { const unsigned long long k = (unsigned long long)sb << 32; if ((k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & dm], 1u); });
        } else {
            sel_sweep(ar, rule, qb, qn, tid, [&](uint32_t sb, uint32_t i) {
                const unsigned long long ks = (unsigned long long)sb << 32;
                if ((ks & mask & 0xFFFFFFFF00000000ull) != (prefix & 0xFFFFFFFF00000000ull)) return;
                const unsigned long long k = ks | (0xFFFFFFFFu - (uint32_t)ar.doc[qb + i]);
                if ((k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & dm], 1u);
            });
        }
        __syncthreads();
        // chunked suffix scan from the top bin: thread t (< 256) owns `per` bins
        const uint32_t per = nb >= 256 ? nb / 256 : 1, nchunks = nb / per;
        if ((uint32_t)tid < nchunks) { uint32_t c = 0; for (uint32_t j = 0; j < per; j++) c += hist[nb - 1 - ((uint32_t)tid * per + j)]; part[tid] = c; }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0, c = 0;
            for (; c < nchunks; c++) { if (acc + part[c] >= remain) break; acc += part[c]; }
            if (c >= nchunks) c = nchunks - 1;
            uint32_t bsel = nb - 1 - (c * per + per - 1);
            for (uint32_t j = 0; j < per; j++) {
                uint32_t bin = nb - 1 - (c * per + j);
                if (acc + hist[bin] >= remain) { bsel = bin; break; }
                acc += hist[bin];
            }
            sBin = bsel; sRemain = remain > acc ? remain - acc : 0; sCount = hist[bsel];
        }
        __syncthreads();
        prefix |= (unsigned long long)sBin << shift; mask |= (unsigned long long)dm << shift;
        remain = sRemain; undecided = sCount;
        if (shift == 4) { shift = 0; width = 4; } else if (shift == 0) shift = -1; else shift -= 12;
        __syncthreads();
    }
    // gather every key >= the undecided range on the decided digits
    if (tid == 0) sCount = 0;
    __syncthreads();
    sel_sweep(ar, rule, qb, qn, tid, [&](uint32_t sb, uint32_t i) {
        const unsigned long long ks = (unsigned long long)sb << 32;
        if (((ks | 0xFFFFFFFFull) & mask) < prefix) { leftMax = max(leftMax, sb); return; }    // cannot reach the undecided range whatever its doc id: skip the doc read
        const unsigned long long k = ks | (0xFFFFFFFFu - (uint32_t)ar.doc[qb + i]);
        if ((k & mask) >= prefix) { uint32_t q2 = atomicAdd(&sCount, 1u); if (q2 < SEL_CAP) keys[q2] = k; }
        else leftMax = max(leftMax, sb);
    });
    }
    // best score among the rows that were not gathered (exact: the cut's ambiguity test needs the best row LEFT OUT, gathered or not)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) leftMax = max(leftMax, (uint32_t)__shfl_xor((int)leftMax, d));
    if ((tid & 63) == 0 && leftMax) atomicMax(&sLeft, leftMax);
    __syncthreads();
    SELP(3);
    const uint32_t n = min(sCount, (uint32_t)SEL_CAP);
    uint32_t cap2 = 64; while (cap2 < n) cap2 <<= 1;           // sort only the next power of two
    for (uint32_t i = n + tid; i < cap2; i += SEL_THREADS) keys[i] = 0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= cap2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < cap2; i += SEL_THREADS) {
                uint32_t ixj = i ^ j;
                if (ixj > i) {
                    unsigned long long a = keys[i], b2 = keys[ixj];
                    bool up = (i & k) == 0;   // descending inside "up" blocks
                    if (up ? (a < b2) : (a > b2)) { keys[i] = b2; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    SELP(4);
#ifdef SEL_PROF
    if (g_selProf && tid == 0) g_selProf[(size_t)q * 8 + 7] = n;
#endif
    const uint32_t take = min(n, (uint32_t)depth);
    for (uint32_t i = tid; i < take; i += SEL_THREADS) {
        unsigned long long k = keys[i];
        infx_hit h; h.doc = (int32_t)(0xFFFFFFFFu - (uint32_t)k); h.score = __uint_as_float((uint32_t)(k >> 32));
        out[(uint64_t)q * outStride + i] = h;
    }
    if (tid == 0) {
        outCount[q] = take;
        // The best row LEFT OUT of the list: the first gathered row after the cut, or — when the gather ended exactly at the cut, or overflowed the sort —
        // the best row that was not gathered (sLeft).  0: every row was taken.
        float nxt = 0.f;
        if (take == (uint32_t)depth) {
            if (n > (uint32_t)depth) nxt = __uint_as_float((uint32_t)(keys[depth] >> 32));
            nxt = fmaxf(nxt, __uint_as_float(sLeft));
            if (sCount > (uint32_t)SEL_CAP) nxt = fmaxf(nxt, __uint_as_float((uint32_t)(keys[depth - 1] >> 32)));      // gathered rows beyond the sort's capacity were dropped unseen (mode 3 never does that; the radix path ends with <= SEL_CAP): bound by the cut
        }
        // Is the cut ambiguous?  The best row left out scores within SEL_AMBIG_REL of the last row taken (exact ties included): the reference's
        // position-dependent fp32 rounding (Q9) and heap order (Q10) decide such cuts — the exact replay handles them.
        if (flagged) {
            bool amb = false; int why = 2;                     // why: 0 exact plateau (equal scores across the cut), 1 inside the band, 2 (no longer produced) left-out row unknown
            if (take == (uint32_t)depth && nxt > 0.f) {
                const float cut = __uint_as_float((uint32_t)(keys[depth - 1] >> 32));
                amb = nxt >= cut * (1.0f - SEL_AMBIG_REL); why = nxt == cut ? 0 : 1;
            }
            flagged[q] = amb ? 1u : 0u;
            if (amb && flagStats) atomicAdd(&flagStats[why], 1u);
        }
        // Document shards: the cut is taken over ALL shards (k_gflag, after the all-gather of these lists), which needs the best first-pass score this
        // shard left out (0 when every row was taken).
        if (nextOut) nextOut[q] = nxt;
    }
    SELP(5);
}
