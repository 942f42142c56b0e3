// Query.highlight on the device: where each returned document matched, the spans a UI paints and a snippet.  Not in the reference (DESIGN.md, "highlight").
// Included by infidex_hip.hip behind stage2.hip.inc, whose helpers (tokeniser, comparisons, distances, the LDS staging scheme) it uses.
//
// ONE launch per batch, one lane per (query, row) slot of the result table, after the post-processing: the rows are the ones that leave.  A lane is inactive
// when its row is past the query's count or its query did not ask.  The wave stages its documents' texts in LDS as k_stage2 does (S2_POOL_CHARS units per
// 64 lanes; a text that does not fit is read from global memory).  The lane then
//   1. tokenises and de-duplicates the document as Stage 2 does (tables of INFX_MAX_DOC_TOKENS entries per lane, as k_stage2's retry launch; more words: HL_TOO_LONG),
//   2. runs the four matchers IN STAGE 2'S ORDER AND WITH ITS CONDITIONS, and at each of the six sites where a query word is matched and taken out of play
//      records (document word, kind, distance, covered part).  The matchers are restated here — k_stage2 and stage2.hip.inc are untouched, so that the kernels
//      of a batch without highlight are byte for byte what they were; tests/test_gpu_highlight.py holds the features these records determine (WordHits,
//      Terms*Matched, FirstMatchIndex, PhraseSpan, the prefix runs, PrecedingStrictCount) to k_stage2's own for every returned row, which keeps the two in step,
//   3. writes the term records, walks the raw words for the spans (hl_span_walk), chooses the window (hl_window) and copies the snippet out (highlight.h).
// The instantiation is the custom-setup one (the matcher settings as a kernel argument; the defaults when the batch has none), alias folding off or on as the
// batch's Stage 2 ran.
#include "highlight.h"      // (HL_FN stays host-and-device: the host sizes the rows with hl_row_u16)
#define HL_THREADS 64

struct DevHighlight {
    const int32_t* slot;        // per query: its index among the asking queries (its rows' place in `out`), -1 = it did not ask
    const int32_t* chars;       // per query: highlight_chars
    const int32_t* docs;        // the result table's documents, `stride` per query
    const uint32_t* counts;     // rows per query
    uint32_t nq, stride;
    uint16_t* out;              // asking queries x stride rows of hl_row_u16(termStride, snipStride)
    uint32_t termStride, snipStride;
    int poolChars;
};

template <bool AL>
__global__ __launch_bounds__(HL_THREADS) void k_highlight(DevIndex ix, const infx_cov_query* __restrict__ queries, DevHighlight H, const infx_stage2_setup cs) {
    constexpr int MAXD = INFX_MAX_DOC_TOKENS, MAXQ = INFX_MAX_QUERY_TOKENS;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x;
    const uint32_t q = gid / H.stride, r = gid - q * H.stride;
    // No early return before the texts are staged: the wave copies them together (inactive lanes contribute length 0).
    bool active = q < H.nq;
    int32_t slot = -1;
    if (active) { slot = H.slot[q]; active = slot >= 0 && r < min(H.counts[q], H.stride); }
    const uint32_t rowU16 = hl_row_u16(H.termStride, H.snipStride);
    uint16_t* row = H.out + (active ? ((size_t)slot * H.stride + r) * rowU16 : 0);
    int32_t doc = 0, gdoc = 0;
    if (active) {
        gdoc = H.docs[gid]; doc = gdoc - ix.docBase;
        for (uint32_t i = 0; i < HL_HDR; i++) row[i] = 0;
        row[6] = (uint16_t)((uint32_t)gdoc & 0xFFFFu); row[7] = (uint16_t)((uint32_t)gdoc >> 16);
        if (doc < 0 || doc >= ix.N) { row[0] = HL_BAD_ROW; active = false; }
    }
    const infx_cov_query* QC = queries + (q < H.nq ? q : 0);
    if (active && QC->reserved != 0) { row[0] = HL_LONG_QUERY; active = false; }
    uint64_t tb = 0; int dlen = 0;
    if (active) { tb = ix.textOff[doc]; dlen = (int)(ix.textOff[doc + 1] - tb); }
    const uint16_t* dptr = ix.text + tb;
    if (H.poolChars > 0) {      // (k_stage2's staging)
        extern __shared__ __attribute__((aligned(16))) uint16_t s2pool[];
        int incl = dlen;
#pragma unroll
        for (int d = 1; d < HL_THREADS; d <<= 1) { const int v = __shfl_up(incl, d); if (lane >= d) incl += v; }
        const int off = incl - dlen;
        const bool fits = active && dlen > 0 && incl <= H.poolChars;
        const int cl = fits ? dlen : 0;
        const uint32_t tlo = (uint32_t)tb, thi = (uint32_t)(tb >> 32);
        unsigned long long todo = __ballot(cl > 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1; todo &= todo - 1;
            const int n = __builtin_amdgcn_readlane(cl, l), o = __builtin_amdgcn_readlane(off, l);
            const uint64_t sb = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)thi, l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)tlo, l);
            const uint16_t* src = ix.text + sb;
            for (int i = lane; i < n; i += HL_THREADS) s2pool[o + i] = src[i];
        }
        __syncthreads();
        if (fits) dptr = (const uint16_t*)(s2pool + off);
    }
    if (!active) return;
    const S2Str Q{QC->text, QC->text_len};
    const S2Str D{dptr, dlen};
    const int qCount = min(max(QC->num_tokens, 0), MAXQ);
    bool over = false, levOver = false;

    uint16_t dOff[MAXD], dLen[MAXD], uOff[MAXD], uLen[MAXD]; uint8_t di[MAXD], uniq[MAXD], termOf[MAXD]; unsigned long long dActive[(MAXD + 63) / 64];
    const int MinWordSize = cs.min_word_size;
    const int dCountRaw = s2_tokenize(D, MinWordSize, dOff, dLen, MAXD, &over);
    if (over) { row[0] = HL_TOO_LONG; return; }
    row[8] = (uint16_t)dCountRaw;
    // dedupe (CoverageTokenizer.DeduplicateDocTokens): the first occurrences, in order; uniq: which of them a raw word equals
#define HDLEN(j) ((int)uLen[j])
#define HDPOS(j) ((int)uOff[j])
#define HDTOK(j) s2_sub(D, HDPOS(j), HDLEN(j))
    int dCount = 0;
    for (int i = 0; i < dCountRaw; i++) {
        const int li = dLen[i];
        S2Str w = s2_sub(D, dOff[i], li);
        int at = -1;
        for (int j = 0; j < dCount; j++) if (HDLEN(j) == li && s2_eq<AL>(s2_sub(D, HDPOS(j), li), w)) { at = j; break; }
        if (at < 0) { uOff[dCount] = dOff[i]; uLen[dCount] = (uint16_t)li; at = dCount++; }
        uniq[i] = (uint8_t)at;
    }
#define HQTOK(i) s2_sub(Q, QC->tok_off[i], QC->tok_len[i])
#define HQLEN(i) ((int)QC->tok_len[i])
    S2QMask<1> qActive; qActive.fill(qCount);
    for (int j = 0; j < (MAXD + 63) / 64; j++) dActive[j] = 0ull;
    for (int j = 0; j < dCount; j++) dActive[j >> 6] |= 1ull << (j & 63);
    float matched[MAXQ];
    // the records: per query word the site that matched it (HL_K_*), the distance, the distinct document word(s), the covered part relative to the word's start
    uint8_t rKind[MAXQ], rDist[MAXQ], rW[MAXQ], rW2[MAXQ]; uint16_t rRel[MAXQ], rMl[MAXQ];
    for (int i = 0; i < qCount; i++) { matched[i] = 0.f; rKind[i] = HL_K_NONE; rDist[i] = 0; rW[i] = 0; rW2[i] = 0; rRel[i] = 0; rMl[i] = 0; }
#define HREC(i, kind, dist, w, w2, rel, ml) do { rKind[i] = (uint8_t)(kind); rDist[i] = (uint8_t)(dist); rW[i] = (uint8_t)(w); rW2[i] = (uint8_t)(w2); rRel[i] = (uint16_t)(rel); rMl[i] = (uint16_t)(ml); } while (0)

    if (qCount > 0) {
        // ---- WholeWordMatcher.Match (site 1) ----
        if (cs.cover_whole_words) {
            for (int i = 0; i < qCount; i++) {
                S2Str qt = HQTOK(i);
                int mi = -1;
                for (int j = 0; j < dCount; j++) if (s2_get(dActive, j) && HDLEN(j) == qt.len && s2_eq<AL>(qt, HDTOK(j))) { mi = j; break; }
                if (mi != -1) {
                    matched[i] += (float)qt.len;
                    HREC(i, HL_K_WHOLE, 0, mi, 0, 0, qt.len);
                    qActive.clr(i); s2_clr(dActive, mi);
                }
            }
        }
        // ---- JoinedWordMatcher.Match (sites 2 and 3) ----
        if (cs.cover_joined_words) {
            for (int i = 0; i < qCount - 1; i++) {
                if (!qActive.test(i) || !qActive.test(i + 1)) continue;
                int next = -1;
                for (int k = i + 1; k < qCount; k++) if (qActive.test(k)) { next = k; break; }
                if (next == -1) break;
                S2Str q1 = HQTOK(i), q2 = HQTOK(next);
                int jl = q1.len + q2.len, mi = -1;
                for (int j = 0; j < dCount; j++) if (s2_get(dActive, j) && HDLEN(j) == jl && s2_starts<AL>(HDTOK(j), q1) && s2_ends<AL>(HDTOK(j), q2)) { mi = j; break; }
                if (mi != -1) {
                    matched[i] += (float)q1.len; matched[next] += (float)q2.len;
                    HREC(i, HL_K_JOINED_QUERY, 0, mi, 0, 0, q1.len);
                    HREC(next, HL_K_JOINED_QUERY, 0, mi, 0, q1.len, q2.len);
                    qActive.clr(i); qActive.clr(next); s2_clr(dActive, mi);
                }
            }
            for (int i = 0; i < dCount - 1; i++) {
                if (!s2_get(dActive, i)) continue;
                int next = -1;
                for (int k = i + 1; k < dCount; k++) if (s2_get(dActive, k)) { next = k; break; }
                if (next == -1) break;
                S2Str d1 = HDTOK(i), d2 = HDTOK(next);
                int jl = d1.len + d2.len, mi = -1;
                for (int j = 0; j < qCount; j++) if (qActive.test(j) && HQLEN(j) == jl && s2_starts<AL>(HQTOK(j), d1) && s2_ends<AL>(HQTOK(j), d2)) { mi = j; break; }
                if (mi != -1) {
                    matched[mi] += (float)jl;
                    HREC(mi, HL_K_JOINED_DOC, 0, i, next, 0, d1.len);
                    qActive.clr(mi); s2_clr(dActive, i); s2_clr(dActive, next);
                }
            }
        }
        // ---- PrefixSuffixMatcher.Match (sites 4 and 5) ----
        if (cs.cover_prefix_suffix) {
            uint8_t qi[MAXQ]; int nqa = 0, nda = 0;
            for (int i = 0; i < qCount; i++) if (qActive.test(i)) qi[nqa++] = (uint8_t)i;
            for (int j = 0; j < dCount; j++) if (s2_get(dActive, j)) di[nda++] = (uint8_t)j;
            for (int a = 1; a < nqa; a++) { int cur = qi[a], cl = HQLEN(cur), j = a - 1; while (j >= 0 && HQLEN(qi[j]) < cl) { qi[j + 1] = qi[j]; j--; } qi[j + 1] = (uint8_t)cur; }
            for (int a = 1; a < nda; a++) { int cur = di[a], cl = HDLEN(cur), j = a - 1; while (j >= 0 && HDLEN(di[j]) < cl) { di[j + 1] = di[j]; j--; } di[j + 1] = (uint8_t)cur; }
            for (int a = 0; a < nqa; a++) {      // MatchExact
                int i = qi[a];
                if (!qActive.test(i)) continue;
                S2Str qt = HQTOK(i); int ql = qt.len;
                for (int bidx = 0; bidx < nda; bidx++) {
                    int j = di[bidx];
                    if (!s2_get(dActive, j)) continue;
                    int dl = HDLEN(j);
                    if (ql == dl) continue;
                    S2Str dt = HDTOK(j);
                    int kind = HL_K_NONE, rel = 0, ml = ql; double ms = 0;
                    if (ql < dl) {
                        int at;
                        if (s2_starts<AL>(dt, qt)) { ms = ql; kind = HL_K_PREFIX; }
                        else if (s2_ends<AL>(dt, qt)) { ms = max(1, ql / 2); kind = HL_K_SUFFIX; rel = dl - ql; }
                        else if (ql >= 4 && (at = s2_index_of<AL>(dt, qt)) >= 0) { ms = ql * 0.6; kind = HL_K_INFIX; rel = at; }
                    } else {
                        if (s2_ends<AL>(qt, dt)) { ms = dl; kind = HL_K_TAIL; ml = dl; }
                    }
                    if (kind != HL_K_NONE) {
                        matched[i] += (float)ms;
                        HREC(i, kind, 0, j, 0, rel, ml);
                        qActive.clr(i); s2_clr(dActive, j);
                        break;
                    }
                }
            }
            for (int a = 0; a < nqa; a++) {      // MatchFuzzyPrefix
                int i = qi[a];
                if (!qActive.test(i)) continue;
                S2Str qt = HQTOK(i); int ql = qt.len;
                if (!(ql >= 4 || (i == qCount - 1 && ql >= 2))) continue;
                for (int bidx = 0; bidx < nda; bidx++) {
                    int j = di[bidx];
                    if (!s2_get(dActive, j)) continue;
                    int dl = HDLEN(j);
                    if (ql >= dl) continue;
                    S2Str dt = HDTOK(j);
                    bool isMatch = false; double ms = 0; int pl = ql;
                    int dist = AL ? min(2, s2_damerau<true>(qt, s2_sub(dt, 0, ql), 1, &levOver)) : s2_dam1(qt, s2_sub(dt, 0, ql));
                    if (dist <= 1) { ms = ql - dist; if (ms < 0.1) ms = 0.1; isMatch = true; }
                    else if (dl > ql) {
                        dist = AL ? min(2, s2_damerau<true>(qt, s2_sub(dt, 0, ql + 1), 1, &levOver)) : s2_dam1(qt, s2_sub(dt, 0, ql + 1));
                        if (dist <= 1) { ms = ql - dist; if (ms < 0.1) ms = 0.1; isMatch = true; pl = ql + 1; }
                        else if (ql > 1) {
                            dist = AL ? min(2, s2_damerau<true>(qt, s2_sub(dt, 0, ql - 1), 1, &levOver)) : s2_dam1(qt, s2_sub(dt, 0, ql - 1));
                            if (dist <= 1) { ms = ql - 1 - dist; if (ms < 0.1) ms = 0.1; isMatch = true; pl = ql - 1; }
                        }
                    }
                    if (isMatch) {
                        matched[i] += (float)ms;
                        HREC(i, HL_K_FUZZY_PREFIX, dist, j, 0, 0, pl);
                        qActive.clr(i); s2_clr(dActive, j);
                        break;
                    }
                }
            }
        }
        // ---- FuzzyWordMatcher.Match (unless all terms fully matched; site 6) ----
        if (cs.cover_fuzzy_words) {
            bool allFull = true;
            for (int i = 0; i < qCount; i++) if (HQLEN(i) > 0 && matched[i] < (float)HQLEN(i)) { allFull = false; break; }
            if (!allFull) {
                const int NumTypos = cs.num_typos, MinLengthOneTypo = cs.min_len_one_typo, MinLengthTwoTypos = cs.min_len_two_typos, LevMaxWord = cs.lev_max_word_size;
                int maxQL = 0;
                for (int i = 0; i < qCount; i++) if (qActive.test(i) && HQLEN(i) > maxQL) maxQL = HQLEN(i);
                if (maxQL != 0) {
                    int maxEd = maxQL >= MinLengthTwoTypos ? 2 : (maxQL >= MinLengthOneTypo ? 1 : 0);
                    if (maxQL == 2 && maxEd == 0 && NumTypos >= 1) maxEd = 1;
                    if (maxEd > NumTypos) maxEd = NumTypos;
                    for (int ed = 1; ed <= maxEd; ed++) {
                        if (!qActive.any()) break;
                        for (int i = 0; i < qCount; i++) {
                            if (!qActive.test(i)) continue;
                            int ql = HQLEN(i);
                            if (ql < MinWordSize) continue;
                            int tme = ql >= MinLengthTwoTypos ? 2 : (ql >= MinLengthOneTypo ? 1 : 0);
                            bool special = false;
                            if (ql == 2 && tme == 0 && NumTypos >= 1) { tme = 1; special = true; }
                            if (tme > NumTypos) tme = NumTypos;
                            if (ed > tme) continue;
                            if (special && ed != 1) continue;
                            int minLen = max(MinWordSize, ql - ed), maxLen = min(LevMaxWord, ql + ed);
                            if (maxLen > 63) maxLen = 63;
                            S2Str qt = HQTOK(i);
                            for (int j = 0; j < dCount; j++) {
                                if (!s2_get(dActive, j)) continue;
                                int dl = HDLEN(j);
                                if (dl > maxLen || dl < minLen) continue;
                                S2Str dt = HDTOK(j);
                                if (special && (dt.len == 0 || dt.p[0] != qt.p[0])) continue;
                                int dist = AL ? s2_damerau<true>(qt, dt, ed, &levOver) : (ed == 1 ? s2_dam1(qt, dt) : s2_damerau(qt, dt, ed, &levOver));
                                if (dist <= ed) {
                                    matched[i] += (float)(ql - dist);
                                    HREC(i, HL_K_FUZZY, dist, j, 0, 0, dl);
                                    qActive.clr(i); s2_clr(dActive, j);
                                    break;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    // ---- the term records; which term each distinct word belongs to (the first, where two query words share it) ----
    for (int j = 0; j < dCount; j++) termOf[j] = HL_NO_TERM;
    uint16_t* T = row + hl_terms_at();
    for (int i = 0; i < qCount; i++) {
        uint16_t tmp[HL_TERM];
        uint16_t* t = (uint32_t)i < H.termStride ? T + (size_t)i * HL_TERM : tmp;      // (the stride is the batch's largest word count: always the first arm)
        const int k = rKind[i];
        if (k == HL_K_NONE) { for (uint32_t c = 0; c < HL_TERM; c++) t[c] = 0; continue; }
        const int w = rW[i], w2 = rW2[i];
        t[0] = (uint16_t)k; t[1] = rDist[i]; t[2] = uOff[w]; t[3] = uLen[w]; t[4] = (uint16_t)(uOff[w] + rRel[i]); t[5] = rMl[i];
        t[6] = k == HL_K_JOINED_DOC ? uOff[w2] : 0; t[7] = k == HL_K_JOINED_DOC ? uLen[w2] : 0;
        if (termOf[w] == HL_NO_TERM) termOf[w] = (uint8_t)i;
        if (k == HL_K_JOINED_DOC && termOf[w2] == HL_NO_TERM) termOf[w2] = (uint8_t)i;
        // in the spans, the words of a joined match are covered whole (the two query words of a joined_query share theirs), as are whole, tail and fuzzy ones
        if (k == HL_K_JOINED_QUERY || k == HL_K_JOINED_DOC || k == HL_K_WHOLE || k == HL_K_TAIL || k == HL_K_FUZZY) { rRel[i] = 0; rMl[i] = HL_WHOLE_WORD; }
    }
    row[1] = (uint16_t)min((uint32_t)qCount, H.termStride);
    // ---- spans, window, snippet ----
    uint16_t* S = row + hl_spans_at(H.termStride);
    bool truncated = false;
    const uint32_t ns = hl_span_walk((uint32_t)dCountRaw, dOff, dLen, uniq, termOf, rRel, rMl, S, &truncated);
    row[2] = (uint16_t)ns; row[3] = truncated ? 1 : 0;
    const uint32_t width = (uint32_t)min(max(H.chars[q], HL_MIN_CHARS), min(HL_MAX_CHARS, (int)H.snipStride));
    const HlWindow Wd = hl_window((uint32_t)dCountRaw, dOff, dLen, S, ns, width);
    const uint32_t sl = min(min(Wd.len, width), (uint32_t)dlen - min(Wd.start, (uint32_t)dlen));
    row[4] = (uint16_t)Wd.start; row[5] = (uint16_t)sl;
    uint16_t* X = row + hl_snippet_at(H.termStride);
    for (uint32_t i = 0; i < sl; i++) X[i] = D.p[Wd.start + i];
#undef HREC
#undef HQLEN
#undef HQTOK
#undef HDTOK
#undef HDPOS
#undef HDLEN
}
