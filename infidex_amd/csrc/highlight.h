// The arithmetic of Query.highlight (k_highlight, highlight.hip.inc): the layout of a highlighted row, the walk over a document's words that lists the spans a UI
// paints, and the choice of the snippet window.  Not in the reference: highlighting is this project's ("highlight").
//
// Plain C++ behind HL_FN, no HIP types: compiled into k_highlight and, unchanged, into a host model that holds the walk and the window to a brute force over
// every window (tests/models/highlight_model.cpp, tests/test_highlight_spans_model.py).  tests/highlight_model.py restates both in Python.
//
// A row (one returned document of one query) is hl_row_u16(T, W) uint16 in a row: T the batch's largest Stage-2 word count, W its largest highlight_chars.
//   header  HL_HDR         [0] status  [1] terms  [2] spans  [3] truncated  [4] snippet_start  [5] snippet_len  [6] [7] document (low, high half)
//                          [8] raw words of the document (DocTokenCount)  [9] 0
//   terms   T x HL_TERM    kind, distance, offset, length, match_offset, match_length, offset2, length2        (one per Stage-2 query word, in its order)
//   spans   64 x HL_SPAN   offset, length, match_offset, match_length, term                                     (ascending offset)
//   snippet W              the UTF-16 units [snippet_start, snippet_start + snippet_len) of the stored text
// Offsets and lengths are UTF-16 units of the stored text (at most 65 535: Stage 2's own tables hold them in 16 bits).
//
// THE WINDOW RULE.  The raw words are the document's words under the batch's MinWordSize, in text order; `width` is the query's highlight_chars.
//   1. A candidate window begins at the word start `a` of a span.  It ends at e = the largest word end with e - a <= width; when not even the span's own word
//      fits (it is longer than width), e = a + width: that word's first `width` units.
//   2. A candidate's rank is (distinct terms among the spans that begin in [a, e), the number of those spans).  The highest rank wins, the earliest candidate
//      among equals.  Without a span the only candidate begins at the first raw word; without a raw word the snippet is empty (start 0, length 0).
//   3. Context: with unused = width - (e - a), the window's start moves left to the EARLIEST raw word start b with a - b <= unused / 4 (integer division); it
//      stays at `a` when there is none.  The end stays, so e - b <= width.  The snippet is [b, e).
#pragma once
#include <stdint.h>
#ifndef HL_FN
#define HL_FN __host__ __device__ __forceinline__
#endif
#define HL_MAX_SPANS 64u
#define HL_MIN_CHARS 16
#define HL_MAX_CHARS 512
#define HL_HDR 10u
#define HL_TERM 8u
#define HL_SPAN 5u
#define HL_NO_TERM 0xFFu                    // a distinct document word no query word matched
#define HL_WHOLE_WORD 0xFFFFu               // a term's match length in the span walk: the whole of every occurrence
// Highlight.status
#define HL_OK 0
#define HL_TOO_LONG 1                       // the document has more than INFX_MAX_DOC_TOKENS Stage-2 words
#define HL_LONG_QUERY 2                     // the query is outside the fast envelope (infx_cov_query.reserved != 0)
#define HL_BAD_ROW 3                        // the row's document is not one of the index (never seen by a caller: the batch fails)
// TermMatch.kind
#define HL_K_NONE 0
#define HL_K_WHOLE 1
#define HL_K_JOINED_QUERY 2
#define HL_K_JOINED_DOC 3
#define HL_K_PREFIX 4
#define HL_K_SUFFIX 5
#define HL_K_INFIX 6
#define HL_K_TAIL 7
#define HL_K_FUZZY_PREFIX 8
#define HL_K_FUZZY 9

HL_FN uint32_t hl_row_u16(uint32_t termStride, uint32_t snipStride) { return HL_HDR + HL_TERM * termStride + HL_SPAN * HL_MAX_SPANS + snipStride; }
HL_FN uint32_t hl_terms_at() { return HL_HDR; }
HL_FN uint32_t hl_spans_at(uint32_t termStride) { return HL_HDR + HL_TERM * termStride; }
HL_FN uint32_t hl_snippet_at(uint32_t termStride) { return HL_HDR + HL_TERM * termStride + HL_SPAN * HL_MAX_SPANS; }

// The span walk.  off / len: the n raw words in text order; uniq[i]: the distinct word (Stage 2's dedupe: first occurrences, alias folding included) raw word
// i equals; termOf[u]: the term that matched distinct word u, HL_NO_TERM for none; rel[t] / mlen[t]: the part of the word term t covers, relative to the
// word's start (mlen HL_WHOLE_WORD: all of it — equal words have equal lengths, so the part carries over to every occurrence).  Writes at most HL_MAX_SPANS
// spans, the first in text order, and returns their number; *truncated: an occurrence was left out.
template <class W, class U, class T, class R>
HL_FN uint32_t hl_span_walk(uint32_t n, const W* off, const W* len, const U* uniq, const T* termOf, const R* rel, const R* mlen, uint16_t* spans, bool* truncated) {
    uint32_t k = 0; *truncated = false;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t t = termOf[uniq[i]];
        if (t == HL_NO_TERM) continue;
        if (k == HL_MAX_SPANS) { *truncated = true; break; }
        uint16_t* s = spans + (size_t)k * HL_SPAN;
        const bool whole = mlen[t] == HL_WHOLE_WORD;
        s[0] = (uint16_t)off[i]; s[1] = (uint16_t)len[i];
        s[2] = (uint16_t)(whole ? off[i] : off[i] + rel[t]); s[3] = (uint16_t)(whole ? len[i] : mlen[t]); s[4] = (uint16_t)t;
        k++;
    }
    return k;
}

struct HlWindow { uint32_t start, len; };
HL_FN uint32_t hl_popc(uint32_t x) { uint32_t c = 0; while (x) { x &= x - 1; c++; } return c; }
// The window rule above.  off / len: the n raw words; spans: ns spans in ascending offset (hl_span_walk's), each beginning at a raw word's start, terms < 32.
template <class W>
HL_FN HlWindow hl_window(uint32_t n, const W* off, const W* len, const uint16_t* spans, uint32_t ns, uint32_t width) {
    HlWindow R; R.start = 0; R.len = 0;
    if (n == 0) return R;
    uint32_t bestA = 0, bestE = 0, bestT = 0, bestS = 0; bool have = false;
    uint32_t j = 0;                                                // the first raw word that ends beyond a + width: only moves right as `a` does
    const uint32_t ncand = ns ? ns : 1u;
    for (uint32_t k = 0; k < ncand; k++) {
        const uint32_t a = ns ? (uint32_t)spans[(size_t)k * HL_SPAN] : (uint32_t)off[0];
        while (j < n && (uint32_t)off[j] + (uint32_t)len[j] <= a + width) j++;
        const uint32_t lastEnd = j > 0 ? (uint32_t)off[j - 1] + (uint32_t)len[j - 1] : 0u;
        const uint32_t e = lastEnd > a ? lastEnd : a + width;     // (no word from `a` on fits: the word at `a` is longer than width)
        uint32_t mask = 0, cnt = 0;
        for (uint32_t m = k; m < ns; m++) {
            if ((uint32_t)spans[(size_t)m * HL_SPAN] >= e) break;
            cnt++; mask |= 1u << (spans[(size_t)m * HL_SPAN + 4] & 31u);
        }
        const uint32_t t = hl_popc(mask);
        if (!have || t > bestT || (t == bestT && cnt > bestS)) { have = true; bestA = a; bestE = e; bestT = t; bestS = cnt; }
    }
    const uint32_t used = bestE - bestA, budget = (width > used ? width - used : 0u) / 4u;
    uint32_t b = bestA;
    for (uint32_t i = 0; i < n && (uint32_t)off[i] < bestA; i++) if (bestA - (uint32_t)off[i] <= budget) { b = (uint32_t)off[i]; break; }
    R.start = b; R.len = bestE - b;
    return R;
}
