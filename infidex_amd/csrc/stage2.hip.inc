// Stage 2 on device — one lane per (query, candidate document).
//
// Replaces the per-candidate body of SearchPipeline.ProcessCandidate (Scoring/SearchPipeline.cs:449-522):
//   SegmentProcessor.CalculateLcs -> StringMetrics.Lcs              (Metrics/StringMetrics.cs:12-36)
//   CoverageEngine.CalculateCoverageInternal                        (Coverage/CoverageEngine.cs:222-382)
//     WholeWordMatcher / JoinedWordMatcher / PrefixSuffixMatcher / FuzzyWordMatcher (Coverage/*.cs)
//     CoverageScorer.CalculateFinalScore                            (Coverage/CoverageScorer.cs:5-198)
//     FusionSignalComputer.ComputeSignals                           (Coverage/FusionSignalComputer.cs:53-568)
//   FusionScorer.Calculate                                          (Scoring/FusionScorer.cs:19-236,313-396)
// Both texts are case-folded before they reach the device (query: SearchEngine.cs:274; documents: at upload), so the
// reference's OrdinalIgnoreCase comparisons are plain code-unit comparisons here.
// Branchy integer/string work: no LDS tiling, per-lane state in registers / scratch; the win over the CPU is width
// (tens of thousands of candidates in flight), not per-lane speed.

#define S2_THREADS 64
#define S2_MAXD INFX_MAX_DOC_TOKENS

#include "s2str.hip.inc"

__device__ __forceinline__ bool s2_is_delim(uint16_t c) {
    // ' ' - / . , : ; ' ` * & \ _ ( ) { } [ ] \t  + U+2013 U+2014   (ConfigurationParameters.cs:58-62)
    if (c < 64) return ((0xc00f7c100000200ull >> c) & 1ull) != 0;
    if (c < 128) return ((0x28000001b8000000ull >> (c - 64)) & 1ull) != 0;
    return c == 0x2013 || c == 0x2014;
}
__device__ __forceinline__ bool s2_is_ws(uint16_t c) {
    return c == 0x20 || (c >= 0x09 && c <= 0x0D) || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
           c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}
// char.IsLetter from data (unicode_tables.h, tools/gen_unicode_tables.py): Lu | Ll | Lt | Lm | Lo of the BMP
__device__ const uint32_t d_ucLetter[2048] = { INFX_UC_LETTER_WORDS };
__device__ __forceinline__ bool s2_is_letter(uint16_t c) {
    if (c < 0x80) return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
    return ((d_ucLetter[c >> 5] >> (c & 31)) & 1u) != 0;
}
// OrdinalIgnoreCase on lower-cased text.  The caller hands over LOWER-cased text (document texts at infx_upload_docs, the coverage queries per batch).  The reference
// compares ToUpperInvariant images at its OrdinalIgnoreCase sites (the four matchers, most of FusionSignalComputer) and plain / ToLowerInvariant characters at the others
// (StringMetrics.Lcs, the transposition scan of CalculateDamerau, FusionSignalComputer.cs:191-228, 427, 457-550, FuzzyWordMatcher.cs:110).  On lower-cased text the two only
// differ for the 22 lower-case characters that share their upper-case image with ANOTHER lower-case character — final sigma / sigma, long s / s, micro sign / mu, the Greek
// symbol forms, Cyrillic Extended-C (`icrep`: class representative lower(upper(c))).  Round 6: the texts stay as they are; infx_upload_docs counts the alias characters of
// the corpus and every batch those of its queries; only when there is one anywhere does Stage 2 run its ALIAS instantiation (template parameter AL), in which the
// OrdinalIgnoreCase sites compare class representatives (s2_fold_ic on both sides) and the other sites the code units — the reference's result at every site.  Without alias
// characters both kinds of site are `==` and the plain instantiation is exact.  (Rounds 4-5 folded the texts in place and compared with `==` everywhere: exact at the
// OrdinalIgnoreCase sites, wrong at the others when an alias met its base letter.)
__device__ const uint16_t d_ucIcrep[INFX_UC_N_ICREP][2] = { INFX_UC_ICREP_PAIRS };
__host__ __device__ __forceinline__ bool s2_alias_range(uint16_t c) {      // a superset of the 22 alias characters, cheap to test
    return !(c < 0xB5 || !(c == 0xB5 || c == 0x17F || (uint32_t)(c - 0x345u) <= 0xB0u || (uint32_t)(c - 0x1C80u) <= 0x33Eu));
}
__device__ __forceinline__ uint16_t s2_fold_ic(uint16_t c) {
    if (!s2_alias_range(c)) return c;
    for (int i = 0; i < INFX_UC_N_ICREP; i++) if (d_ucIcrep[i][0] == c) return d_ucIcrep[i][1];
    return c;
}
#define S2_FOLD(c) s2_fold_ic(c)
// alias characters in a text (the corpus at upload): *count += their number
__global__ void k_count_alias(const uint16_t* __restrict__ text, unsigned long long n, unsigned long long* __restrict__ count) {
    unsigned long long c = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) { const uint16_t ch = text[i]; if (s2_fold_ic(ch) != ch) c++; }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}
static const uint16_t h_ucIcrep[INFX_UC_N_ICREP][2] = { INFX_UC_ICREP_PAIRS };
static inline bool s2_host_is_alias(uint16_t c) {
    if (!s2_alias_range(c)) return false;
    for (int i = 0; i < INFX_UC_N_ICREP; i++) if (h_ucIcrep[i][0] == c) return h_ucIcrep[i][1] != c;
    return false;
}
// F: compare OrdinalIgnoreCase class representatives (the ALIAS instantiation at the reference's OrdinalIgnoreCase sites); else code units
template <bool F = false> __device__ __forceinline__ bool s2_ceq(uint16_t x, uint16_t y) { return F ? (x == y || s2_fold_ic(x) == s2_fold_ic(y)) : x == y; }
template <bool F = false> __device__ __forceinline__ bool s2_eq(S2Str a, S2Str b) {
    if (a.len != b.len) return false;
    for (int i = 0; i < a.len; i++) if (!s2_ceq<F>(a.p[i], b.p[i])) return false;
    return true;
}
template <bool F = false> __device__ __forceinline__ bool s2_starts(S2Str s, S2Str p) {
    if (s.len < p.len) return false;
    for (int i = 0; i < p.len; i++) if (!s2_ceq<F>(s.p[i], p.p[i])) return false;
    return true;
}
template <bool F = false> __device__ __forceinline__ bool s2_ends(S2Str s, S2Str p) {
    if (s.len < p.len) return false;
    const uint16_t* b = s.p + (s.len - p.len);
    for (int i = 0; i < p.len; i++) if (!s2_ceq<F>(b[i], p.p[i])) return false;
    return true;
}
template <bool F = false> __device__ __forceinline__ int s2_index_of(S2Str s, S2Str p) {
    if (p.len == 0) return 0;
    for (int i = 0; i + p.len <= s.len; i++) {
        int j = 0; while (j < p.len && s2_ceq<F>(s.p[i + j], p.p[j])) j++;
        if (j == p.len) return i;
    }
    return -1;
}

#include "lev.hip.inc"

// tokenise into (off,len) pairs; returns count, sets *over when more than cap tokens qualify
__device__ int s2_tokenize(S2Str t, int minWordSize, uint16_t* off, uint16_t* len, int cap, bool* over) {
    int n = t.len, i = 0, cnt = 0;
    while (i < n) {
        while (i < n && s2_is_delim(t.p[i])) i++;
        if (i >= n) break;
        int st = i;
        while (i < n && !s2_is_delim(t.p[i])) i++;
        int L = i - st;
        if (L >= minWordSize) {
            if (cnt < cap) { off[cnt] = (uint16_t)st; len[cnt] = (uint16_t)min(L, 65535); cnt++; }
            else *over = true;
        }
    }
    return cnt;
}

// "still unmatched" set over the document's distinct tokens: one bit per token
__device__ __forceinline__ bool s2_get(const unsigned long long* b, int i) { return (b[i >> 6] >> (i & 63)) & 1ull; }
__device__ __forceinline__ void s2_clr(unsigned long long* b, int i) { b[i >> 6] &= ~(1ull << (i & 63)); }

// MAXD = capacity of the per-lane document token tables.  The first launch runs with S2_FASTD (the tables then fit in registers /
// a small scratch frame); a row whose document has more tokens is marked S2_RETRY and redone by the second launch (MAXD = S2_MAXD),
// whose other lanes exit at once.
#define S2_FASTD 32
#ifndef S2_MIN_WAVES
#define S2_MIN_WAVES 6      // waves per SIMD the register allocation must allow (<= 80 VGPRs; measured 2: 7.3 ms, 4: 5.1 ms, 6: 4.5 ms per batch)
#endif
#define S2_RETRY 0xFE
#define S2_RETRY2 0xFD
// Long queries (infx_cov_query.reserved != 0: beyond INFX_MAX_QUERY_TOKENS words / INFX_MAX_QUERY_CHARS characters): the first launch marks their rows S2_RETRYQ,
// the LQ instantiations (query tables of INFX_LONGQ_TOKENS entries, four mask words instead of one) redo them — S2_MAXD-token documents first, the rest
// (S2_RETRY2Q) through the global-workspace pass.  Same code, same results; only these rows pay for the larger per-lane tables.
#define S2_RETRYQ 0xFC
#define S2_RETRY2Q 0xFB
// one bit per query word: "still unmatched" / matched by a whole word / joined / as a prefix
template <int NW> struct S2QMask {
    uint32_t w[NW];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < NW; k++) w[k] = 0u;
    }
    __device__ __forceinline__ void fill(int n) {      // bits 0 .. n-1
#pragma unroll
        for (int k = 0; k < NW; k++) { const int r = n - 32 * k; w[k] = r >= 32 ? 0xFFFFFFFFu : (r <= 0 ? 0u : ((1u << r) - 1u)); }
    }
    __device__ __forceinline__ bool test(int i) const { return NW == 1 ? ((w[0] >> i) & 1u) != 0 : ((w[i >> 5] >> (i & 31)) & 1u) != 0; }
    __device__ __forceinline__ void set(int i) { if (NW == 1) w[0] |= 1u << i; else w[i >> 5] |= 1u << (i & 31); }
    __device__ __forceinline__ void clr(int i) { if (NW == 1) w[0] &= ~(1u << i); else w[i >> 5] &= ~(1u << (i & 31)); }
    __device__ __forceinline__ bool any() const { uint32_t a = 0;
#pragma unroll
        for (int k = 0; k < NW; k++) a |= w[k];
        return a != 0; }
};
// Third launch (HUGE): documents beyond S2_MAXD words.  The reference accepts texts up to 65 535 characters (Api/DocumentFields.cs:140), i.e. up to
// 32 768 tokens; their token tables do not fit a lane's registers or scratch, so a row of this pass carves them out of a global pool: the second
// launch leaves the document's token count in the row, the third allocates 5 * n + n / 16 uint16 (offsets, lengths, the distinct tokens' offsets and lengths, the
// length-sorted index list, the unmatched bit set) with one atomic.  Same code, same results, only slower (the reference's quadratic de-duplication
// runs on one lane): no envelope on the document length; a batch whose over-long rows exceed the pool flags the rest (result flag bit 3).
#define S2_HUGE_TOKENS 32768
__device__ int s2_count_tokens(S2Str t) {                    // non-empty tokens: an upper bound for both tokenisations (MinWordSize 2 and 0)
    int n = t.len, i = 0, cnt = 0;
    while (i < n) { while (i < n && s2_is_delim(t.p[i])) i++; if (i >= n) break; while (i < n && !s2_is_delim(t.p[i])) i++; cnt++; }
    return cnt;
}
#ifndef S2_LDS_ULEN
#define S2_LDS_ULEN 0        // 1: the fast launch keeps the distinct tokens' lengths (clipped to a byte) in LDS, 2 KB per 64-candidate workgroup.  Measured (GPU call 20):
                             // the compact tables alone 6.32 -> 5.69 ms (config 3) / 1.66 -> 1.48 ms (config 4); with the LDS lengths 7.06 / 1.88 ms at the 3072-unit text pool
                             // and 6.13 / 1.74 ms at 2048 — the 2 KB cost a wave of occupancy per SIMD, more than the cheaper rejections give back.  Off.
#endif
#ifndef S2_POOL_CHARS
#define S2_POOL_CHARS 3072   // 6 KB of LDS per 64-candidate workgroup (measured on the 10M-doc batch: 0 -> 2.21 ms, 2048 -> 2.00, 3072 -> 1.84, 4096 -> 2.03, 6144 -> 2.47: larger pools cost occupancy)
#endif
// CS: the "custom setup" instantiations.  The engine-wide matcher settings of CoverageSetup (infx_stage2_setup: MinWordSize — also minStemLength of the fusion
// signals —, the five Cover* switches, the three typo thresholds, LevenshteinMaxWordSize) arrive as the kernel argument `cs` (uniform: scalar registers) instead of
// being the literals of CoverageSetup.cs:6-103.  Without CS every one of them folds to its default at compile time and `cs` is never read: those instantiations
// compile to what they were before the argument existed.  The fast launch has a plain and an ALIAS custom instantiation (the ALIAS form forgoes the one-pass
// distance-1 Damerau and folds at every comparison: half as fast again); the retry, huge-pool and the two long-query launches — a few rows of a batch — only the ALIAS
// one, which is exact with or without alias characters: six kernels more, not ten.
template <int MAXD, int MINW, bool HUGE = false, bool LQ = false, bool AL = false, bool CS = false>
__global__ __launch_bounds__(S2_THREADS, MINW) void k_stage2(DevIndex ix, const infx_cov_query* __restrict__ queries, uint32_t nq,
                                                        const infx_cov_cand* __restrict__ cands, uint32_t ncand,
                                                        infx_cov_out* __restrict__ outs, int32_t* __restrict__ featOut, int globalIds, int retryPass,
                                                        const int32_t* __restrict__ pairs, int poolChars,
                                                        uint16_t* __restrict__ hugeWs = nullptr, uint32_t* __restrict__ hugeCounter = nullptr, uint32_t hugeUnits = 0,
                                                        const infx_cov_query_long* __restrict__ longq = nullptr, uint32_t nLong = 0,
                                                        const infx_stage2_setup cs = infx_stage2_setup{}) {
    constexpr int LOC = HUGE ? 1 : MAXD;                              // per-lane table capacity held in registers / scratch
    constexpr int MAXQ = LQ ? INFX_LONGQ_TOKENS : INFX_MAX_QUERY_TOKENS;      // capacity of the per-lane query-word tables
    typedef typename std::conditional<LQ, infx_cov_query_long, infx_cov_query>::type QCT;
    typedef S2QMask<MAXQ / 32> QM;
    typedef typename std::conditional<(HUGE || MAXD > 255), uint16_t, uint8_t>::type idx_t;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x;
    // No early return before the document texts are staged: the wave copies them together (inactive lanes contribute length 0).
    bool active = gid < ncand;
    infx_cov_cand C; C.query = 0xFFFFFFFFu; C.doc = 0; C.base_score = 0.f; C.want_lcs = 0;
    if (active) { C = cands[gid]; if (C.query == 0xFFFFFFFFu) active = false; }       // unused row of a strided (per-query) candidate table
    // pairs (fused pipeline): -2 = this row is derived by its partner's lane, >= 0 = row that shares this row's document and differs
    // only in base_score (a Stage-1 document that is also a WordMatcher hit)
    int32_t partner = -1;
    if (active) { partner = pairs ? pairs[gid] : -1; if (partner == -2) active = false; }
    if (active && retryPass && outs[gid].status != (LQ ? (HUGE ? S2_RETRY2Q : S2_RETRYQ) : (HUGE ? S2_RETRY2 : S2_RETRY))) active = false;
    if (active && globalIds) {                          // sharded: rows carry global ids; a shard scores the documents it holds, the rest stay 0
        C.doc -= ix.docBase;
        if (C.doc < 0 || C.doc >= ix.N) { infx_cov_out Z; Z.score = 0.f; Z.tiebreaker = 0; Z.word_hits = 0; Z.lcs = 0; Z.status = 0; Z.word_hits_full = 0; outs[gid] = Z; active = false; }
    }
    infx_cov_out O;
    O.score = 0.f; O.tiebreaker = 0; O.word_hits = 0; O.lcs = 0; O.status = 0; O.word_hits_full = 0;
    if (active && (C.query >= nq || C.doc < 0 || C.doc >= ix.N)) { O.status = INFX_EINVAL; outs[gid] = O; if (featOut) for (int i = 0; i < INFX_NFEAT; i++) featOut[(size_t)gid * INFX_NFEAT + i] = 0; active = false; }
    int lqi = 0;                                        // 1 + index of the query's record in the long-query table, 0 = a query of the fast envelope
    if (active) lqi = queries[C.query].reserved;
    if (!LQ && active && lqi != 0) {                    // (first launch only: the later launches of the fast envelope pick their rows by status)
        O.status = (lqi > 0 && (uint32_t)lqi <= nLong) ? S2_RETRYQ : INFX_EINVAL; outs[gid] = O; if (partner >= 0) outs[partner] = O; active = false;
    }
    if (LQ && active && (lqi <= 0 || (uint32_t)lqi > nLong)) active = false;
    uint64_t tb = 0; int dlen = 0;
    if (active) { tb = ix.textOff[C.doc]; dlen = (int)(ix.textOff[C.doc + 1] - tb); }
    const uint16_t* dptr = ix.text + tb;
    // ---- document texts into LDS -----------------------------------------------------------------------------------------
    // Every later pass (tokeniser, four matchers, fusion signals) reads the text character by character, each lane a different document:
    // from global memory that is one 2-byte load per lane per step, 64 cache lines per wave instruction.  The wave instead copies its
    // documents once, row by row with coalesced loads, into a pool of poolChars UTF-16 units; a lane whose text does not fit (pool full)
    // keeps reading global memory — S2Str holds generic pointers, so both kinds of lane run the same code.
    if (poolChars > 0) {
        extern __shared__ __attribute__((aligned(16))) uint16_t s2pool[];
        int incl = dlen;
#pragma unroll
        for (int d = 1; d < S2_THREADS; d <<= 1) { const int v = __shfl_up(incl, d); if (lane >= d) incl += v; }
        const int off = incl - dlen;
        const bool fits = active && dlen > 0 && incl <= poolChars;
        const int cl = fits ? dlen : 0;
        const uint32_t tlo = (uint32_t)tb, thi = (uint32_t)(tb >> 32);
        unsigned long long todo = __ballot(cl > 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1; todo &= todo - 1;
            const int n = __builtin_amdgcn_readlane(cl, l), o = __builtin_amdgcn_readlane(off, l);
            const uint64_t sb = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)thi, l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)tlo, l);
            const uint16_t* src = ix.text + sb;
            for (int i = lane; i < n; i += S2_THREADS) s2pool[o + i] = src[i];
        }
        __syncthreads();
        if (fits) dptr = (const uint16_t*)(s2pool + off);
    }
    if (!active) return;
    const QCT* QC;
    if constexpr (LQ) QC = longq + (lqi - 1); else QC = queries + C.query;
    const S2Str Q{QC->text, QC->text_len};
    const S2Str D{dptr, dlen};
    const int qCount = QC->num_tokens;
    bool over = false, levOver = false;
    float score2 = 0.f;

    // ---- LCS for docIndex < 2 (quirk Q7) --------------------------------------------------------------------------
    int lcs = 0;
    if (C.want_lcs) {
        if (Q.len > 0 && D.len > 0) {
            if (s2_eq(Q, D) || s2_index_of(D, Q) >= 0) lcs = Q.len;
            else {
                int prefix = 0, len = min(Q.len, D.len);
                for (int i = 0; i < len; i++) { if (Q.p[i] != D.p[i]) break; prefix++; }
                lcs = prefix == 0 ? 0 : min(prefix + QC->lcs_tolerance, len);
            }
        }
        if (C.want_lcs == 2) lcs = min(lcs, 255);      // this row IS the document's second evaluation (rows handed over one by one: infx_cov_cand.want_lcs)
        O.lcs = (uint8_t)min(lcs, 255);
    }
    const bool wholeQuery = !CS || cs.cover_whole_query != 0;      // !CoverWholeQuery: the coverage score ignores the LCS (CoverageEngine.cs:269); the row keeps it for the truncation
    double lcsSum = wholeQuery ? (double)lcs : 0.0;
    // Quirk Q18 (SearchPipeline.cs:492-503): the LCS of docIndex 0 / 1 is kept in a BYTE span; a document evaluated twice — overlap row, then Stage-1 row — reads it
    // back for its second evaluation, so a value above 255 (queries longer than 255 characters contained in the document) comes back as 255.  The partner row
    // derived below is that second evaluation: where the two values differ, the features the LCS feeds (CoverageScore's fallback, the single-term SumCi) and the
    // score are computed a second time for it.
    const int lcsP = min(lcs, 255);
    const bool split = partner >= 0 && lcsP != lcs;
    const double lcsSumP = wholeQuery ? (double)lcsP : 0.0;
    uint8_t CoverageScoreP = 0; float SumCiP = 0.f;

    // feature state
    int wordHits = 0, docTokenCount = 0;
    int TermsWithAnyMatch = 0, TermsFullyMatched = 0, TermsStrictMatched = 0, TermsPrefixMatched = 0, FirstMatchIndex = -1;
    int LongestPrefixRun = 0, SuffixPrefixRun = 0, PhraseSpan = 0, PrecedingStrictCount = 0;
    bool LastTokenHasPrefix = false, LastTermIsTypeAhead = false;
    float SumCi = 0.f, LastTermCi = 0.f, WeightedCoverage = 0.f, IdfCoverage = 0.f, TotalIdf = 0.f, MissingIdf = 0.f;
    uint8_t CoverageScore = 0;
    float termCi[MAXQ];
    // fusion signals
    int fUnf = 0; bool fPrefixLast = false, fAllPrecExact = false, fPerfect = false, fStem = false, fAnchor = false;
    uint8_t fTrailing = 0, fSingleSim = 0; int fSingleChar = 0;

    uint16_t dOffL[LOC], dLenL[LOC], uOffL[LOC], uLenL[LOC]; idx_t diL[LOC]; unsigned long long actL[HUGE ? 1 : (MAXD + 63) / 64];
    uint16_t *dOff = dOffL, *dLen = dLenL;     // raw doc tokens (MinWordSize 2); reused for fusion tokens later
    uint16_t *uOff = uOffL, *uLen = uLenL;     // the distinct ones (first occurrences), compact: the matchers' loops read a token with ONE table access
    idx_t* di = diL; unsigned long long* dActive = actL;
    // The length of a distinct token is what every matcher loop tests first (and mostly rejects on): the fast launch keeps it — clipped to a byte — in LDS, one column
    // per lane, so that the common rejection costs an LDS read instead of a scratch (memory) access.  255 = "255 or longer: look it up".
    constexpr bool LT = S2_LDS_ULEN != 0 && !HUGE && MAXD == S2_FASTD;
    __shared__ uint8_t s2ulen[LT ? S2_FASTD * S2_THREADS : 1];
    int cap = MAXD;                             // capacity of the token tables
    if (HUGE) {                                 // tables of this row in the global pool, sized by the token count the second launch left in the row
        cap = min(S2_HUGE_TOKENS, (outs[gid].word_hits_full + 3) & ~3);
        const uint32_t units = (uint32_t)(5 * cap + ((cap + 63) / 64) * 4 + 4);
        const uint32_t off = atomicAdd(hugeCounter, units);
        if (cap <= 0 || (unsigned long long)off + units > (unsigned long long)hugeUnits) {      // pool exhausted by this batch's over-long rows: flagged, not scored
            O.status = INFX_EUNSUPPORTED; outs[gid] = O; if (partner >= 0) outs[partner] = O; return;
        }
        uint16_t* w = hugeWs + off;
        dOff = w; dLen = w + cap; uOff = w + 2 * cap; uLen = w + 3 * cap; di = (idx_t*)(w + 4 * cap); dActive = (unsigned long long*)(w + 5 * cap);
    }

    if (qCount > 0) {
        const int MinWordSize = CS ? cs.min_word_size : 2;
        int dCountRaw = s2_tokenize(D, MinWordSize, dOff, dLen, cap, &over);
        docTokenCount = dCountRaw;
        // dedupe (CoverageTokenizer.DeduplicateDocTokens): the first occurrences, in order
#define DLEN(j) (LT ? (s2ulen[(j) * S2_THREADS + lane] < 255 ? (int)s2ulen[(j) * S2_THREADS + lane] : (int)uLen[j]) : (int)uLen[j])
#define DPOS(j) ((int)uOff[j])
#define DTOK(j) s2_sub(D, DPOS(j), DLEN(j))
        int dCount = 0;
        for (int i = 0; i < dCountRaw; i++) {
            const int li = dLen[i];
            S2Str cs = s2_sub(D, dOff[i], li);
            bool dup = false;
            for (int j = 0; j < dCount; j++) if (DLEN(j) == li && s2_eq<AL>(s2_sub(D, DPOS(j), li), cs)) { dup = true; break; }
            if (!dup) { uOff[dCount] = dOff[i]; uLen[dCount] = (uint16_t)li; if (LT) s2ulen[dCount * S2_THREADS + lane] = (uint8_t)min(li, 255); dCount++; }
        }
#define QTOK(i) s2_sub(Q, QC->tok_off[i], QC->tok_len[i])
#define QLEN(i) ((int)QC->tok_len[i])
        QM qActive; qActive.fill(qCount);
        for (int j = 0; j < (dCount + 63) / 64; j++) dActive[j] = 0ull;
        for (int j = 0; j < dCount; j++) dActive[j >> 6] |= 1ull << (j & 63);
        QM hasWhole, hasJoined, hasPrefix; hasWhole.clear(); hasJoined.clear(); hasPrefix.clear();
        float matched[MAXQ]; int firstPos[MAXQ];
        for (int i = 0; i < qCount; i++) { matched[i] = 0.f; firstPos[i] = -1; termCi[i] = 0.f; }
        double numWhole = 0, numJoined = 0, numFuzzy = 0, numPS = 0; int penalty = 0;
#define SETPOS(i, pos) do { int p_ = (pos); if (firstPos[i] == -1 || p_ < firstPos[i]) firstPos[i] = p_; } while (0)

        // ---- WholeWordMatcher.Match ----
        if (!CS || cs.cover_whole_words) {
            int pInc = qCount > 1 ? 1 : 0;
            for (int i = 0; i < qCount; i++) {
                S2Str qt = QTOK(i);
                int mi = -1;
                for (int j = 0; j < dCount; j++) if (s2_get(dActive, j) && DLEN(j) == qt.len && s2_eq<AL>(qt, DTOK(j))) { mi = j; break; }
                if (mi != -1) {
                    wordHits++; numWhole += qt.len;
                    matched[i] += (float)qt.len; hasWhole.set(i); hasPrefix.set(i);
                    SETPOS(i, DPOS(mi));
                    if (dCount > i) { if (DLEN(i) != qt.len || !s2_eq<AL>(qt, DTOK(i))) penalty++; } else penalty++;
                    if (i < qCount - 1) numWhole += pInc;
                    qActive.clr(i); s2_clr(dActive, mi);
                }
            }
        }
        // ---- JoinedWordMatcher.Match ----
        if (!CS || cs.cover_joined_words) {
            for (int i = 0; i < qCount - 1; i++) {
                if (!qActive.test(i) || !qActive.test(i + 1)) continue;
                int next = -1;
                for (int k = i + 1; k < qCount; k++) if (qActive.test(k)) { next = k; break; }
                if (next == -1) break;
                S2Str q1 = QTOK(i), q2 = QTOK(next);
                int jl = q1.len + q2.len, mi = -1;
                for (int j = 0; j < dCount; j++) if (s2_get(dActive, j) && DLEN(j) == jl && s2_starts<AL>(DTOK(j), q1) && s2_ends<AL>(DTOK(j), q2)) { mi = j; break; }
                if (mi != -1) {
                    numJoined += jl; wordHits += 2;
                    matched[i] += (float)q1.len; hasJoined.set(i); hasPrefix.set(i);
                    int pos = DPOS(mi); SETPOS(i, pos);
                    matched[next] += (float)q2.len; hasJoined.set(next); SETPOS(next, pos);
                    qActive.clr(i); qActive.clr(next); s2_clr(dActive, mi);
                }
            }
            for (int i = 0; i < dCount - 1; i++) {
                if (!s2_get(dActive, i)) continue;
                int next = -1;
                for (int k = i + 1; k < dCount; k++) if (s2_get(dActive, k)) { next = k; break; }
                if (next == -1) break;
                S2Str d1 = DTOK(i), d2 = DTOK(next);
                int jl = d1.len + d2.len, mi = -1;
                for (int j = 0; j < qCount; j++) if (qActive.test(j) && QLEN(j) == jl && s2_starts<AL>(QTOK(j), d1) && s2_ends<AL>(QTOK(j), d2)) { mi = j; break; }
                if (mi != -1) {
                    numJoined += jl; wordHits += 1;
                    matched[mi] += (float)jl; hasJoined.set(mi); hasPrefix.set(mi);
                    SETPOS(mi, DPOS(i));
                    qActive.clr(mi); s2_clr(dActive, i); s2_clr(dActive, next);
                }
            }
        }
        // ---- PrefixSuffixMatcher.Match ----
        if (!CS || cs.cover_prefix_suffix) {
            uint8_t qi[MAXQ]; int nqa = 0, nda = 0;
            for (int i = 0; i < qCount; i++) if (qActive.test(i)) qi[nqa++] = (uint8_t)i;
            for (int j = 0; j < dCount; j++) if (s2_get(dActive, j)) di[nda++] = (idx_t)j;
            for (int a = 1; a < nqa; a++) { int cur = qi[a], cl = QLEN(cur), j = a - 1; while (j >= 0 && QLEN(qi[j]) < cl) { qi[j + 1] = qi[j]; j--; } qi[j + 1] = (uint8_t)cur; }
            for (int a = 1; a < nda; a++) { int cur = di[a], cl = DLEN(cur), j = a - 1; while (j >= 0 && DLEN(di[j]) < cl) { di[j + 1] = di[j]; j--; } di[j + 1] = (idx_t)cur; }
            for (int a = 0; a < nqa; a++) {      // MatchExact
                int i = qi[a];
                if (!qActive.test(i)) continue;
                S2Str qt = QTOK(i); int ql = qt.len;
                for (int bidx = 0; bidx < nda; bidx++) {
                    int j = di[bidx];
                    if (!s2_get(dActive, j)) continue;
                    int dl = DLEN(j);
                    if (ql == dl) continue;
                    S2Str dt = DTOK(j);
                    bool isMatch = false, isPrefix = false; double ms = 0;
                    if (ql < dl) {
                        if (s2_starts<AL>(dt, qt)) { ms = ql; isMatch = true; isPrefix = true; }
                        else if (s2_ends<AL>(dt, qt)) { ms = max(1, ql / 2); isMatch = true; }
                        else if (ql >= 4 && s2_index_of<AL>(dt, qt) >= 0) { ms = ql * 0.6; isMatch = true; }
                    } else {
                        if (s2_ends<AL>(qt, dt)) { ms = dl; isMatch = true; }
                    }
                    if (isMatch) {
                        numPS += ms; wordHits++;
                        matched[i] += (float)ms; if (isPrefix) hasPrefix.set(i);
                        SETPOS(i, DPOS(j));
                        qActive.clr(i); s2_clr(dActive, j);
                        break;
                    }
                }
            }
            for (int a = 0; a < nqa; a++) {      // MatchFuzzyPrefix
                int i = qi[a];
                if (!qActive.test(i)) continue;
                S2Str qt = QTOK(i); int ql = qt.len;
                if (!(ql >= 4 || (i == qCount - 1 && ql >= 2))) continue;
                for (int bidx = 0; bidx < nda; bidx++) {
                    int j = di[bidx];
                    if (!s2_get(dActive, j)) continue;
                    int dl = DLEN(j);
                    if (ql >= dl) continue;
                    S2Str dt = DTOK(j);
                    bool isMatch = false; double ms = 0;
                    int dist = AL ? min(2, s2_damerau<true>(qt, s2_sub(dt, 0, ql), 1, &levOver)) : s2_dam1(qt, s2_sub(dt, 0, ql));
                    if (dist <= 1) { ms = ql - dist; if (ms < 0.1) ms = 0.1; isMatch = true; }
                    else if (dl > ql) {
                        dist = AL ? min(2, s2_damerau<true>(qt, s2_sub(dt, 0, ql + 1), 1, &levOver)) : s2_dam1(qt, s2_sub(dt, 0, ql + 1));
                        if (dist <= 1) { ms = ql - dist; if (ms < 0.1) ms = 0.1; isMatch = true; }
                        else if (ql > 1) {
                            dist = AL ? min(2, s2_damerau<true>(qt, s2_sub(dt, 0, ql - 1), 1, &levOver)) : s2_dam1(qt, s2_sub(dt, 0, ql - 1));
                            if (dist <= 1) { ms = ql - 1 - dist; if (ms < 0.1) ms = 0.1; isMatch = true; }
                        }
                    }
                    if (isMatch) {
                        numPS += ms; wordHits++;
                        matched[i] += (float)ms;
                        SETPOS(i, DPOS(j));
                        qActive.clr(i); s2_clr(dActive, j);
                        break;
                    }
                }
            }
        }
        // ---- FuzzyWordMatcher.Match (unless all terms fully matched) ----
        if (!CS || cs.cover_fuzzy_words) {
            bool allFull = true;
            for (int i = 0; i < qCount; i++) if (QLEN(i) > 0 && matched[i] < (float)QLEN(i)) { allFull = false; break; }
            if (!allFull) {
                const int NumTypos = CS ? cs.num_typos : 2, MinLengthOneTypo = CS ? cs.min_len_one_typo : 3, MinLengthTwoTypos = CS ? cs.min_len_two_typos : 7, LevMaxWord = CS ? cs.lev_max_word_size : 20;
                int maxQL = 0;
                for (int i = 0; i < qCount; i++) if (qActive.test(i) && QLEN(i) > maxQL) maxQL = QLEN(i);
                if (maxQL != 0) {
                    int maxEd = maxQL >= MinLengthTwoTypos ? 2 : (maxQL >= MinLengthOneTypo ? 1 : 0);
                    if (maxQL == 2 && maxEd == 0 && NumTypos >= 1) maxEd = 1;
                    if (maxEd > NumTypos) maxEd = NumTypos;
                    for (int ed = 1; ed <= maxEd; ed++) {
                        if (!qActive.any()) break;
                        for (int i = 0; i < qCount; i++) {
                            if (!qActive.test(i)) continue;
                            int ql = QLEN(i);
                            if (ql < MinWordSize) continue;
                            int tme = ql >= MinLengthTwoTypos ? 2 : (ql >= MinLengthOneTypo ? 1 : 0);
                            bool special = false;
                            if (ql == 2 && tme == 0 && NumTypos >= 1) { tme = 1; special = true; }
                            if (tme > NumTypos) tme = NumTypos;
                            if (ed > tme) continue;
                            if (special && ed != 1) continue;
                            int minLen = max(MinWordSize, ql - ed), maxLen = min(LevMaxWord, ql + ed);
                            if (maxLen > 63) maxLen = 63;
                            S2Str qt = QTOK(i);
                            for (int j = 0; j < dCount; j++) {
                                if (!s2_get(dActive, j)) continue;
                                int dl = DLEN(j);
                                if (dl > maxLen || dl < minLen) continue;
                                S2Str dt = DTOK(j);
                                if (special && (dt.len == 0 || dt.p[0] != qt.p[0])) continue;
                                int dist = AL ? s2_damerau<true>(qt, dt, ed, &levOver) : (ed == 1 ? s2_dam1(qt, dt) : s2_damerau(qt, dt, ed, &levOver));      // (distance 1: one pass instead of the band, lev.hip.inc)
                                if (dist <= ed) {
                                    wordHits++; numFuzzy += (ql - dist);
                                    matched[i] += (float)(ql - dist);
                                    SETPOS(i, DPOS(j));
                                    qActive.clr(i); s2_clr(dActive, j);
                                    break;
                                }
                            }
                        }
                    }
                }
            }
        }
        // ---- CoverageScorer.CalculateFinalScore ----
        {
            int queryLen = Q.len;
            double num11 = numJoined + numWhole + numFuzzy + numPS - (double)penalty;
            if (split) { double n2 = num11; if (n2 == 0.0 && lcsSumP > 2.0) n2 = lcsSumP - 2.0; CoverageScoreP = (uint8_t)(long long)fmin(n2 / (double)queryLen * 255.0, 255.0); }
            if (num11 == 0.0 && lcsSum > 2.0) num11 = lcsSum - 2.0;
            double v = fmin(num11 / (double)queryLen * 255.0, 255.0);
            CoverageScore = (uint8_t)(long long)v;
            float wsum = 0.f, totalW = 0.f, idfW = 0.f, lastIdf = 0.f;
            int minPos = 0x7FFFFFFF, maxPos = -1;
            for (int i = 0; i < qCount; i++) {
                int mc = QLEN(i);
                if (mc <= 0) continue;
                float ci = fminf(1.0f, matched[i] / (float)mc);
                SumCi += ci; termCi[i] = ci;
                if (ci > 0) TermsWithAnyMatch++;
                float tw = (float)mc; totalW += tw; wsum += ci * tw;
                float idf = QC->term_idf[i];
                TotalIdf += idf; idfW += ci * idf;
                if (ci < 1.0f) MissingIdf += (1.0f - ci) * idf;
                if (i == qCount - 1) { LastTermCi = ci; lastIdf = idf; }
                bool full = matched[i] >= ((float)mc - 0.01f);
                if (full) TermsFullyMatched++;
                if ((hasWhole.test(i) || hasJoined.test(i)) && full) TermsStrictMatched++;
                if (hasPrefix.test(i)) TermsPrefixMatched++;
                if (firstPos[i] >= 0) {
                    if (FirstMatchIndex == -1 || firstPos[i] < FirstMatchIndex) FirstMatchIndex = firstPos[i];
                    if (firstPos[i] < minPos) minPos = firstPos[i];
                    if (firstPos[i] > maxPos) maxPos = firstPos[i];
                }
            }
            WeightedCoverage = totalW > 0.f ? wsum / totalW : 0.f;
            IdfCoverage = TotalIdf > 0.f ? idfW / TotalIdf : 0.f;
            if (qCount > 0 && TotalIdf > 0.f) { float share = lastIdf / TotalIdf; float thr = 1.f / (float)(qCount + 1); LastTermIsTypeAhead = share <= thr; }
            if (split) { SumCiP = SumCi; if (qCount == 1 && queryLen > 0 && lcsSumP > 0.0) { float ciL = (float)fmin(1.0, lcsSumP / (double)queryLen); if (ciL > SumCiP) SumCiP = ciL; } }
            if (qCount == 1 && queryLen > 0 && lcsSum > 0.0) { float ciL = (float)fmin(1.0, lcsSum / (double)queryLen); if (ciL > SumCi) SumCi = ciL; }
            int run = 0;
            for (int i = 0; i < qCount; i++) {
                bool ph = hasPrefix.test(i) && QLEN(i) > 0 && matched[i] > 0;
                if (ph) { run++; if (run > LongestPrefixRun) LongestPrefixRun = run; } else run = 0;
            }
            int srun = 0;
            for (int i = qCount - 1; i >= 0; i--) { bool ph = hasPrefix.test(i) && QLEN(i) > 0 && matched[i] > 0; if (ph) srun++; else break; }
            SuffixPrefixRun = srun;
            if (minPos != 0x7FFFFFFF && maxPos >= minPos && TermsWithAnyMatch >= 2) PhraseSpan = (maxPos - minPos) + 1;
            int li = qCount - 1;
            LastTokenHasPrefix = hasPrefix.test(li) && matched[li] > 0;
            if (qCount >= 2) for (int i = 0; i < qCount - 1; i++) if ((hasWhole.test(i) || hasJoined.test(i)) && matched[i] >= ((float)QLEN(i) - 0.01f)) PrecedingStrictCount++;
        }
        // ---- FusionSignalComputer.ComputeSignals on unfiltered tokens (minWordSize 0; doc tokens re-tokenised) ----
        {
            const int fq = QC->num_fusion_tokens;
            int fd = s2_tokenize(D, 0, dOff, dLen, cap, &over);
            fUnf = fq;
#define FQ(i) s2_sub(Q, QC->ftok_off[i], QC->ftok_len[i])
#define FD(j) s2_sub(D, dOff[j], dLen[j])
            if (fq > 0 && fd > 0) {
                // 1. CheckPrefixLastMatch
                if (fq == 1) {
                    S2Str q0 = FQ(0);
                    for (int i = 0; i < fd; i++) if (s2_starts<AL>(FD(i), q0)) { fPrefixLast = true; fAllPrecExact = s2_eq<AL>(FD(i), q0); break; }
                } else {
                    bool allExact = true;
                    for (int i = 0; i < fq - 1; i++) {
                        S2Str qx = FQ(i);
                        if (qx.len == 0) continue;
                        bool found = false;
                        for (int j = 0; j < fd; j++) if (s2_eq<AL>(FD(j), qx)) { found = true; break; }
                        if (!found) { allExact = false; break; }
                    }
                    if (allExact) {
                        S2Str last = FQ(fq - 1);
                        if (last.len == 0) { fPrefixLast = true; fAllPrecExact = true; }
                        else for (int i = 0; i < fd; i++) if (s2_starts<AL>(FD(i), last)) { fPrefixLast = true; fAllPrecExact = true; break; }
                    }
                }
                // 2. ComputePerfectDoc
                {
                    bool perfect = true;
                    for (int j = 0; j < fd && perfect; j++) {
                        bool explained = false; S2Str dx = FD(j);
                        for (int i = 0; i < fq; i++) { S2Str qx = FQ(i); if (s2_starts<AL>(dx, qx) || s2_starts<AL>(qx, dx)) { explained = true; break; } }
                        if (!explained) perfect = false;
                    }
                    fPerfect = perfect;
                }
                // 3. CheckStemEvidence (minStemLength = MinWordSize = 2, CoverageEngine.cs:376)
                if (fq >= 2) {
                    const int minStem = CS ? cs.min_word_size : 2; int unmatched = 0, evidence = 0;
                    for (int qi2 = 0; qi2 < fq; qi2++) {
                        S2Str qx = FQ(qi2);
                        if (qx.len < minStem) continue;
                        bool wm = false;
                        for (int dj = 0; dj < fd; dj++) { S2Str dx = FD(dj); if (dx.len == 0) continue; if (s2_starts<AL>(dx, qx)) { wm = true; break; } }
                        if (wm) continue;
                        unmatched++;
                        for (int dj = 0; dj < fd; dj++) {
                            S2Str dx = FD(dj);
                            if (dx.len < minStem) continue;
                            if (s2_starts<AL>(qx, dx)) { evidence++; break; }
                            int maxCheck = min(qx.len, dx.len);
                            if (maxCheck >= minStem) {
                                int pl = 0;
                                for (int i = 0; i < maxCheck; i++) { if (qx.p[i] == dx.p[i]) pl++; else break; }
                                if (pl >= minStem) { evidence++; break; }
                            }
                        }
                    }
                    fStem = unmatched > 0 && evidence == unmatched;
                }
                // 4. HasAnchorStem (no DocumentMetadataCache on a freshly indexed engine, see oracle/coverage.hpp)
                if (QC->ftok_len[0] >= 3) {
                    S2Str stem = s2_sub(Q, QC->ftok_off[0], 3);
                    for (int i = 0; i < fd; i++) { S2Str dx = FD(i); if (dx.len >= 3 && s2_starts<AL>(dx, stem)) { fAnchor = true; break; } }
                }
                // 5. TrailingMatchDensity
                if (fq >= 2) {
                    int ll = QC->ftok_len[fq - 1];
                    if (ll >= 1 && ll <= 2) {
                        S2Str lq = FQ(fq - 1); int matchable = 0;
                        for (int i = 0; i < fd; i++) { S2Str dx = FD(i); if (s2_starts<AL>(dx, lq) || (dx.len > lq.len && s2_index_of<AL>(dx, lq) >= 0)) matchable++; }
                        if (matchable > 0) { float dens = (float)matchable / (float)fd; float vv = dens * 255.f; vv = fminf(fmaxf(vv, 0.f), 255.f); fTrailing = (uint8_t)vv; }
                    }
                }
                // 6. SingleTermLexicalSim
                if (fq == 1) {
                    S2Str ql = FQ(0); int qLen = ql.len; float best = 0.f;
                    if (qLen >= 3) {
                        for (int t = 0; t < fd; t++) {
                            S2Str tl = FD(t);
                            if (tl.len < 2) continue;
                            int idx = s2_index_of(ql, tl);
                            if (idx >= 0) {
                                float lenFrac = (float)tl.len / (float)qLen, posF = 1.f - (float)idx / (float)qLen, sc = lenFrac * posF;
                                if (sc > best) best = sc;
                                continue;
                            }
                            int maxK = min(qLen, tl.len), bestK = 0;
                            for (int len = maxK; len >= 2; len--) if (s2_eq(s2_sub(ql, qLen - len, len), s2_sub(tl, 0, len))) { bestK = len; break; }
                            float ps = bestK > 0 ? (float)bestK / (float)qLen : 0.f, fz = 0.f;
                            if (tl.len <= 32) { int dist = s2_damerau(ql, tl, 2, &levOver); if (dist <= 2) fz = (float)(qLen - dist) / (float)qLen; }
                            float comb = fmaxf(ps, fz);
                            if (comb > best) best = comb;
                        }
                        if (qLen >= 6) {
                            int segLen = min(6, qLen / 2);
                            S2Str pf = s2_sub(ql, 0, segLen), sf = s2_sub(ql, qLen - segLen, segLen);
                            int pi = -1, si = -1;
                            for (int i = 0; i < fd; i++) {
                                S2Str tl = FD(i);
                                if (tl.len < 3) continue;
                                if (pi == -1 && (s2_starts(tl, pf) || s2_starts(pf, tl))) pi = i;
                                if (si == -1 && (s2_ends(tl, sf) || s2_ends(sf, tl))) si = i;
                                if (pi != -1 && si != -1) break;
                            }
                            if (pi != -1 && si != -1 && pi != si) { float two = fminf(1.f, (float)(pf.len + sf.len) / (float)qLen); if (two > best) best = two; }
                        }
                    }
                    float vv = best * 255.f; vv = fminf(fmaxf(vv, 0.f), 255.f); fSingleSim = (uint8_t)vv;
                }
                // 7. SingleCharLastTokenBoost
                if (fq >= 2 && QC->ftok_len[fq - 1] == 1) {
                    uint16_t target = Q.p[QC->ftok_off[fq - 1]];
                    if (s2_is_letter(target)) {
                        int dIndex = 0, firstMatch = -1; bool ok = true;
                        for (int i = 0; i < fq - 1 && ok; i++) {
                            S2Str qTerm = FQ(i); bool found = false;
                            while (dIndex < fd) { if (s2_index_of<AL>(FD(dIndex), qTerm) >= 0) { found = true; if (firstMatch == -1) firstMatch = dIndex; break; } dIndex++; }
                            if (!found) ok = false;
                        }
                        if (ok && dIndex + 1 < fd) {
                            S2Str nx = FD(dIndex + 1);
                            if (nx.len > 0 && nx.p[0] == target) {
                                int endOfLast = dOff[dIndex] + dLen[dIndex]; bool broken = false;
                                for (int p = endOfLast; p < (int)dOff[dIndex + 1]; p++) if (!s2_is_ws(D.p[p])) { broken = true; break; }
                                if (!broken) { int boost = 8 + max(0, 16 - firstMatch); if (nx.len == 1) boost += 4; fSingleChar = boost; }
                            }
                        }
                    }
                }
            }
        }
    }

    // ---- FusionScorer.Calculate ---------------------------------------------------------------------------------------
    const int TermsCount = qCount;
    {
        int n = fUnf > 0 ? fUnf : TermsCount;
        bool single = n <= 1;
        bool isComplete = TermsCount > 0 && TermsWithAnyMatch == TermsCount;
        bool isClean = TermsCount > 0 && TermsPrefixMatched == TermsCount;
        bool isExact = TermsCount > 0 && TermsStrictMatched == TermsCount;
        bool startsAtBeginning = FirstMatchIndex == 0;
        int precedingTerms = max(0, TermsCount - 1);
        bool coveragePrefixLast = TermsCount >= 1 && PrecedingStrictCount == precedingTerms && LastTokenHasPrefix;
        bool isPrefixLastStrong = fPrefixLast && coveragePrefixLast;
        int precedence = 0, tier = 0;
        if (!single && TermsCount > 0) {
            int m = TermsWithAnyMatch, tot = TermsCount;
            if (m >= tot) tier = 3; else if (m == tot - 1) tier = 2; else if (m * 2 >= tot) tier = 1; else tier = 0;
        }
        if (!single && tier > 0) precedence |= (tier & 3) << 16;
        bool isExactPrefix = !single && isClean && startsAtBeginning && fPrefixLast && isComplete;
        bool isSubset = !single && docTokenCount > 0 && wordHits == docTokenCount;
        if (isExactPrefix) precedence |= (1 << 15);
        if (isSubset) precedence |= (1 << 14);
        float avgIdf = 0.f;
        const bool arrays = QC->has_word_idf != 0 && TermsCount > 0;
        if (!single && TermsCount >= 2) {
            bool hasDominant = false;
            if (arrays) {
                avgIdf = (TotalIdf > 0.f && TermsCount > 0) ? TotalIdf / (float)TermsCount : 0.f;
                for (int c = 0; c < TermsCount; c++) {
                    float wi = QC->word_idf[c];
                    float power = wi * termCi[c];
                    if (termCi[c] <= 0.1f || wi <= 0.f || wi < avgIdf) continue;
                    float other = 0.f;
                    for (int i = 0; i < TermsCount; i++) if (i != c) other += QC->word_idf[i] * termCi[i];
                    if (power >= other) { hasDominant = true; break; }
                }
            }
            bool strongAnchor = fAnchor && arrays && QC->word_idf[0] >= avgIdf;
            if (hasDominant || strongAnchor) precedence |= (1 << 13);
            int unmatched = TermsCount - TermsWithAnyMatch;
            if (hasDominant && unmatched == 1) precedence |= 8;
        }
        if (single) {
            if (isComplete) precedence |= (1 << 17);
            if (isClean && TermsCount > 0) precedence |= (1 << 16);
            int t = 0;
            if (isComplete) { if (startsAtBeginning) { if (isExact) t = 4; else if (isClean) t = 3; } else { if (isExact) t = 2; else if (isClean) t = 1; } }
            precedence |= t << 3;
        } else {
            bool anchorRun = fAnchor && LongestPrefixRun >= 2;
            int mt = isPrefixLastStrong ? 3 : (fPrefixLast ? 2 : ((fPerfect || anchorRun) ? 1 : 0));
            if (fUnf > TermsCount) mt += fSingleChar;
            precedence |= mt;
        }
        float coverageRatio = TermsCount > 0 ? (float)TermsWithAnyMatch / (float)TermsCount : 0.f;
        bool partial = coverageRatio > 0.f && coverageRatio < 1.f;
        if (partial && n >= 2) {
            if (fStem) precedence |= 8;
            else {
                int unmatched = TermsCount - TermsWithAnyMatch;
                bool lastMatched = LastTokenHasPrefix || (TermsCount > 0 && TermsWithAnyMatch == TermsCount);
                bool canBoost = (lastMatched || !LastTermIsTypeAhead) && TotalIdf > 0.f;
                if (unmatched == 1 && canBoost) {
                    float missRatio = MissingIdf / TotalIdf, gap = 1.f - coverageRatio;
                    if (missRatio < gap) precedence |= 8;
                }
            }
        }
        auto semantic_of = [&](float avgCi) -> float {       // the semantic score before the base-score blend, as a function of the mean per-term coverage
            float sem;
            if (single) { float ls = (float)fSingleSim / 255.f; sem = (avgCi + ls) / 2.f; }
            else if (docTokenCount == 0) sem = avgCi;
            else {
                int unmatched = TermsCount - TermsWithAnyMatch;
                bool lastMatched = LastTokenHasPrefix || (TermsCount > 0 && TermsWithAnyMatch == TermsCount);
                bool canUseIdf = (lastMatched || !LastTermIsTypeAhead) && TotalIdf > 0.f;
                bool useIdf = partial && unmatched == 1 && canUseIdf && IdfCoverage > coverageRatio;
                float base = useIdf ? IdfCoverage : avgCi;
                float density = (float)wordHits / (float)docTokenCount;
                sem = base * density;
                if (TermsCount >= 3) { int sc = (fAnchor ? 1 : 0) + (SuffixPrefixRun >= 2 ? 1 : 0); if (sc > 0) { float bonus = 0.15f * (float)sc; sem = fminf(1.f, sem + bonus); } }
                if (TermsCount >= 2) { float md = (float)fTrailing / 255.f; if (md > 0.f) { float head = 1.f - sem; sem += head * md; } }
            }
            return sem;
        };
        float semantic = semantic_of(TermsCount > 0 ? SumCi / (float)TermsCount : 0.f);
        float gap = 1.f - coverageRatio;
        if (partner >= 0) {                                  // the same document under its other base score (and, quirk Q18, its byte-sized LCS)
            const float b2 = cands[partner].base_score;
            float s2v = split ? semantic_of(TermsCount > 0 ? SumCiP / (float)TermsCount : 0.f) : semantic;
            if (partial && b2 >= gap) s2v = coverageRatio * s2v + gap * b2;
            if (s2v < 0.f) s2v = 0.f;
            if (s2v > 0.999f) s2v = 0.999f;
            score2 = (float)precedence + s2v;
        }
        if (partial && C.base_score >= gap) semantic = coverageRatio * semantic + gap * C.base_score;
        if (semantic < 0.f) semantic = 0.f;
        if (semantic > 0.999f) semantic = 0.999f;
        uint8_t tie = 0;
        if (n >= 2 && D.len > 0) { float focus = fminf(1.f, (float)Q.len / (float)D.len); tie = (uint8_t)(focus * 255.f); }
        O.score = (float)precedence + semantic;
        O.tiebreaker = tie;
    }
    O.word_hits = (uint8_t)min(wordHits, 255);
    O.word_hits_full = wordHits;
    if (over && !HUGE) {                        // token tables too small: the next launch (S2_MAXD, then the global-workspace pass) redoes the row
        infx_cov_out Z; Z.score = 0.f; Z.tiebreaker = 0; Z.word_hits = 0; Z.lcs = 0; Z.status = LQ ? S2_RETRY2Q : (MAXD < S2_MAXD ? S2_RETRY : S2_RETRY2);
        Z.word_hits_full = MAXD < S2_MAXD ? 0 : s2_count_tokens(D);      // the third launch sizes its tables with it
        outs[gid] = Z;
        if (partner >= 0 && MAXD >= S2_MAXD) outs[partner] = Z;      // a partner row left at status 0 / score 0 would enter the ranking: it waits with its row
        return;
    }
    if (over || levOver) O.status = INFX_EUNSUPPORTED;
    if (featOut) {
        int32_t* F = featOut + (size_t)gid * INFX_NFEAT;
        for (int i = 0; i < INFX_NFEAT; i++) F[i] = 0;
        F[0] = CoverageScore; F[1] = TermsCount; F[2] = TermsWithAnyMatch; F[3] = TermsFullyMatched;
        F[4] = TermsStrictMatched; F[5] = TermsPrefixMatched; F[6] = qCount > 0 ? FirstMatchIndex : -1; F[7] = wordHits;
        F[8] = docTokenCount; F[9] = LongestPrefixRun; F[10] = SuffixPrefixRun; F[11] = PhraseSpan;
        F[12] = PrecedingStrictCount; F[13] = LastTokenHasPrefix; F[14] = LastTermIsTypeAhead;
        F[15] = fUnf; F[16] = fPrefixLast; F[17] = fAllPrecExact; F[18] = fPerfect; F[19] = fStem; F[20] = fAnchor;
        F[21] = fTrailing; F[22] = fSingleSim; F[23] = fSingleChar; F[24] = lcs;
        F[25] = __float_as_int(SumCi); F[26] = __float_as_int(IdfCoverage); F[27] = __float_as_int(TotalIdf);
        F[28] = __float_as_int(MissingIdf); F[29] = __float_as_int(LastTermCi); F[30] = __float_as_int(WeightedCoverage);
    }
    outs[gid] = O;
    if (partner >= 0) {
        infx_cov_out O2 = O; O2.score = score2; outs[partner] = O2;
        if (featOut) {
            int32_t* F2 = featOut + (size_t)partner * INFX_NFEAT;
            for (int i = 0; i < INFX_NFEAT; i++) F2[i] = featOut[(size_t)gid * INFX_NFEAT + i];
            if (split) { F2[0] = CoverageScoreP; F2[24] = lcsP; F2[25] = __float_as_int(SumCiP); }
        }
    }
}
