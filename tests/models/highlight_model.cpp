// Host model of the span walk and the window choice of Query.highlight (infidex_amd/csrc/highlight.h, unchanged): hl_span_walk and hl_window on constructed
// word tables, held to a brute force — the spans to a plain recount, the window to an enumeration of EVERY (start word, end word) pair that begins at a span
// and fits the width, ranked as the rule ranks them, and to a plain search for the context start.
// Prints "OK <cases>"; any difference prints the case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <random>
#include <set>
#include <vector>
#define HL_FN static inline
#include "highlight.h"

struct Doc {
    std::vector<uint16_t> text, off, len, rel, mlen;      // rel / mlen: per term
    std::vector<uint8_t> uniq, termOf;                    // termOf: per distinct word
};
struct Span { uint32_t off, len, moff, mlen, term; };

static bool is_high(uint16_t c) { return c >= 0xD800 && c <= 0xDBFF; }

// n words of 2 .. 9 units (or `longWord` units for word `longAt`), some ending in a surrogate pair, some equal to an earlier word; `marked` of them matched,
// spread over the text; terms: 0 = every matched word by term 0, 1 = by distinct terms (mod 32)
static Doc make_doc(std::mt19937& rng, uint32_t n, uint32_t marked, int terms, int longAt, uint32_t longWord) {
    Doc D; D.rel.assign(32, 0); D.mlen.assign(32, HL_WHOLE_WORD);
    for (uint32_t t = 0; t < 32; t++) { const uint32_t k = rng() % 3; if (k == 1) { D.rel[t] = 0; D.mlen[t] = 1; } else if (k == 2) { D.rel[t] = 1; D.mlen[t] = 1; } }
    std::vector<uint32_t> order(n); for (uint32_t i = 0; i < n; i++) order[i] = i;
    for (uint32_t i = n; i > 1; i--) std::swap(order[i - 1], order[rng() % i]);
    std::vector<uint8_t> mark(n, 0); for (uint32_t i = 0; i < marked && i < n; i++) mark[order[i]] = 1;
    uint32_t nuniq = 0, nextTerm = 0;
    for (uint32_t i = 0; i < n; i++) {
        for (uint32_t g = 1 + rng() % 3; g > 0; g--) D.text.push_back(' ');
        uint32_t L = 2 + rng() % 8; int dupOf = -1;
        if ((int)i == longAt) L = longWord;
        else if (i > 0 && rng() % 4 == 0) { const uint32_t j = rng() % i; if ((int)j != longAt && mark[j] == mark[i]) { dupOf = (int)j; L = D.len[j]; } }
        D.off.push_back((uint16_t)D.text.size()); D.len.push_back((uint16_t)L);
        for (uint32_t k = 0; k < L; k++) D.text.push_back((uint16_t)('a' + rng() % 26));
        if (L >= 4 && rng() % 3 == 0) { D.text[D.text.size() - 2] = 0xD83D; D.text[D.text.size() - 1] = 0xDE00; }      // the word ends in a surrogate pair
        if (dupOf >= 0) { D.uniq.push_back(D.uniq[dupOf]); continue; }
        D.uniq.push_back((uint8_t)nuniq++);
        D.termOf.push_back(mark[i] ? (uint8_t)(terms == 0 ? 0 : (nextTerm++ % 32)) : (uint8_t)HL_NO_TERM);
    }
    D.text.push_back('.');
    return D;
}

static int check(const Doc& D, uint32_t width, const char* what) {
    const uint32_t n = (uint32_t)D.off.size();
    // ---- the span walk against a recount ----
    std::vector<uint16_t> S(HL_MAX_SPANS * HL_SPAN + 1, 0xABCD); bool truncated = false;
    const uint32_t ns = hl_span_walk(n, D.off.data(), D.len.data(), D.uniq.data(), D.termOf.data(), D.rel.data(), D.mlen.data(), S.data(), &truncated);
    if (S[HL_MAX_SPANS * HL_SPAN] != 0xABCD) { printf("%s: the walk wrote past its 64 spans\n", what); return 1; }
    std::vector<Span> all;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t t = D.termOf[D.uniq[i]];
        if (t == HL_NO_TERM) continue;
        Span s{D.off[i], D.len[i], D.off[i], D.len[i], t};
        if (D.mlen[t] != HL_WHOLE_WORD) { s.moff = D.off[i] + D.rel[t]; s.mlen = D.mlen[t]; }
        all.push_back(s);
    }
    const uint32_t want = all.size() > HL_MAX_SPANS ? HL_MAX_SPANS : (uint32_t)all.size();
    if (ns != want || truncated != (all.size() > HL_MAX_SPANS)) { printf("%s: %u spans, truncated %d; want %u of %zu\n", what, ns, (int)truncated, want, all.size()); return 1; }
    for (uint32_t k = 0; k < ns; k++) {
        const uint16_t* s = S.data() + k * HL_SPAN;
        if (s[0] != all[k].off || s[1] != all[k].len || s[2] != all[k].moff || s[3] != all[k].mlen || s[4] != all[k].term) { printf("%s: span %u differs\n", what, k); return 1; }
        if (k && s[0] <= S[(k - 1) * HL_SPAN]) { printf("%s: spans not ascending\n", what); return 1; }
    }
    all.resize(ns);
    // ---- the window against every (start word, end word) pair ----
    const HlWindow W = hl_window(n, D.off.data(), D.len.data(), S.data(), ns, width);
    uint32_t a = 0, e = 0; bool have = false;
    if (n) {
        uint32_t bt = 0, bs = 0;
        for (uint32_t s = 0; s < n; s++) {
            bool cand = ns == 0 ? s == 0 : false;
            for (const Span& x : all) if (x.off == D.off[s]) cand = true;
            if (!cand) continue;
            std::vector<uint32_t> ends;
            for (uint32_t t = s; t < n; t++) if ((uint32_t)D.off[t] + D.len[t] - D.off[s] <= width) ends.push_back((uint32_t)D.off[t] + D.len[t]);
            if (ends.empty()) ends.push_back((uint32_t)D.off[s] + width);                       // the word at s alone is longer than the width
            for (uint32_t en : ends) {
                std::set<uint32_t> terms; uint32_t cnt = 0;
                for (const Span& x : all) if (x.off >= D.off[s] && x.off < en) { cnt++; terms.insert(x.term); }
                const uint32_t tt = (uint32_t)terms.size();
                const bool better = !have || tt > bt || (tt == bt && cnt > bs) || (tt == bt && cnt == bs && D.off[s] == a && en > e);
                if (better) { have = true; bt = tt; bs = cnt; a = D.off[s]; e = en; }
            }
        }
        const uint32_t budget = (width > e - a ? width - (e - a) : 0) / 4;
        uint32_t b = a;
        for (uint32_t i = 0; i < n; i++) if (D.off[i] < a && a - D.off[i] <= budget && D.off[i] < b) b = D.off[i];
        a = b;
    }
    if (W.start != a || W.len != e - a) { printf("%s width %u: window [%u, +%u), brute force [%u, +%u)\n", what, width, W.start, W.len, a, e - a); return 1; }
    if (W.len > width || W.start + W.len > D.text.size()) { printf("%s: window out of bounds\n", what); return 1; }
    // a window never cuts a surrogate pair, unless it is the first `width` units of one over-long word
    bool wordEnd = W.len == 0; for (uint32_t i = 0; i < n; i++) if ((uint32_t)D.off[i] + D.len[i] == W.start + W.len) wordEnd = true;
    if (wordEnd && W.len && is_high(D.text[W.start + W.len - 1])) { printf("%s: the window ends inside a surrogate pair\n", what); return 1; }
    if (!wordEnd && W.len != width) { printf("%s: a window that ends inside a word is not `width` long\n", what); return 1; }
    return 0;
}

int main() {
    const uint32_t counts[] = {0, 1, 2, 63, 64, 65, 191, 192}, marks[] = {0, 1, 63, 64, 65}, widths[] = {16, 160, 512};
    std::mt19937 rng(20260317u);
    unsigned long cases = 0;
    char what[128];
    for (uint32_t n : counts) for (uint32_t m : marks) for (int terms = 0; terms < 2; terms++) for (int rep = 0; rep < 3; rep++) {
        const Doc D = make_doc(rng, n, m, terms, -1, 0);
        for (uint32_t w : widths) { snprintf(what, sizeof what, "words %u marked %u terms %d rep %d", n, m, terms, rep); if (check(D, w, what)) return 1; cases++; }
    }
    // a word longer than the width: matched and not, first, in the middle and last
    for (uint32_t w : widths) for (int at : {0, 5, 9}) for (uint32_t m : {0u, 10u}) {
        const Doc D = make_doc(rng, 10, m, 1, at, w + 1 + rng() % 40);
        snprintf(what, sizeof what, "long word at %d marked %u", at, m); if (check(D, w, what)) return 1; cases++;
    }
    // one word that is the whole text, longer than every width
    { const Doc D = make_doc(rng, 1, 1, 0, 0, 600); for (uint32_t w : widths) { if (check(D, w, "one long word")) return 1; cases++; } }
    printf("OK %lu\n", cases);
    return 0;
}
