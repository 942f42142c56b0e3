"""A plain Python restatement of Query.highlight (infidex_amd/csrc/highlight.hip.inc, highlight.h): Stage 2's tokeniser and dedupe, its four matchers with a
record at each of the six sites where a query word is matched and taken out of play, the span walk and the window rule.  Texts are lists of UTF-16 code
units, so offsets mean what the device's mean.  test_highlight_model.py pins it to the oracle; the GPU tests hold the kernel to it field for field.

features(...) derives the Stage-2 coverage features that the records determine; both the model test and the GPU cross-check against k_stage2 use it."""
import numpy as np

DELIMS = frozenset(ord(c) for c in " -/.,:;'`*&\\_(){}[]\t–—")
KINDS = ("none", "whole", "joined_query", "joined_doc", "prefix", "suffix", "infix", "tail", "fuzzy_prefix", "fuzzy")
MAX_DOC_WORDS, MAX_QUERY_WORDS, MAX_QUERY_CHARS, MAX_SPANS = 192, 32, 512, 64
FEATURES = ("WordHits", "TermsWithAnyMatch", "TermsFullyMatched", "TermsStrictMatched", "TermsPrefixMatched", "FirstMatchIndex", "PhraseSpan",
            "LongestPrefixRun", "SuffixPrefixRun", "PrecedingStrictCount", "DocTokenCount")


class Setup:
    """infx_stage2_setup: CoverageSetup's matcher members and their defaults."""
    def __init__(self, min_word_size=2, lev_max_word_size=20, num_typos=2, min_len_one_typo=3, min_len_two_typos=7,
                 cover_whole_words=True, cover_fuzzy_words=True, cover_joined_words=True, cover_prefix_suffix=True):
        self.min_word_size = min_word_size; self.lev_max_word_size = lev_max_word_size; self.num_typos = num_typos
        self.min_len_one_typo = min_len_one_typo; self.min_len_two_typos = min_len_two_typos
        self.cover_whole_words = cover_whole_words; self.cover_fuzzy_words = cover_fuzzy_words
        self.cover_joined_words = cover_joined_words; self.cover_prefix_suffix = cover_prefix_suffix


def units(s):
    return [int(x) for x in np.frombuffer(s.encode("utf-16-le", "surrogatepass"), np.uint16)]


def text_of(u):
    return np.asarray(u, np.uint16).tobytes().decode("utf-16-le", "surrogatepass")


def fold(c):
    """OrdinalIgnoreCase class representative of one code unit: characters with one upper-case image compare equal (final sigma / sigma, ...)."""
    if c < 0x80 or 0xD800 <= c <= 0xDFFF:
        return c
    up = chr(c).upper()
    return ord(up) if len(up) == 1 and ord(up) < 0x10000 else c


def eq(a, b):
    return len(a) == len(b) and all(fold(x) == fold(y) for x, y in zip(a, b))


def starts(s, p):
    return len(s) >= len(p) and eq(s[:len(p)], p)


def ends(s, p):
    return len(s) >= len(p) and eq(s[len(s) - len(p):], p)


def index_of(s, p):
    if not p:
        return 0
    for i in range(len(s) - len(p) + 1):
        if eq(s[i:i + len(p)], p):
            return i
    return -1


def lev(a, b, max_err):
    """Levenshtein distance on folded units, max_err + 1 when it is larger."""
    a = [fold(x) for x in a]; b = [fold(x) for x in b]
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = prev[j - 1] if a[i - 1] == b[j - 1] else min(prev[j], cur[j - 1], prev[j - 1]) + 1
        prev = cur
    return min(prev[len(b)], max_err + 1)


def damerau(a, b, maxd):
    """LevenshteinDistance.CalculateDamerau as Stage 2 states it (lev.hip.inc): the plain distance, and one adjacent transposition at the FIRST mismatch."""
    if abs(len(a) - len(b)) > maxd:
        return maxd + 1
    d = lev(a, b, maxd + 1)
    if d <= maxd:
        return d
    for i in range(len(a) - 1):
        if i >= len(b):
            break
        if a[i] != b[i]:
            if i + 1 < len(b) and a[i] == b[i + 1] and a[i + 1] == b[i]:
                budget = maxd - 1
                if budget < 0:
                    return maxd + 1
                rest = lev(a[i + 2:], b[i + 2:], budget)
                if rest <= budget:
                    return 1 + rest
            break
    return d


def tokenize(u, min_word_size):
    out = []; i = 0; n = len(u)
    while i < n:
        while i < n and u[i] in DELIMS:
            i += 1
        if i >= n:
            break
        st = i
        while i < n and u[i] not in DELIMS:
            i += 1
        if i - st >= min_word_size:
            out.append((st, i - st))
    return out


def dedupe(u, toks):
    """The first occurrences in order, and for every token the distinct one it equals."""
    uniq = []; which = []
    for off, ln in toks:
        at = -1
        for j, (o, l) in enumerate(uniq):
            if l == ln and eq(u[o:o + l], u[off:off + ln]):
                at = j
                break
        if at < 0:
            uniq.append((off, ln)); at = len(uniq) - 1
        which.append(at)
    return uniq, which


def query_words(qu, setup):
    """The query's Stage-2 words (PrepareQuery: MinWordSize-filtered, de-duplicated), or None for a query outside the fast envelope."""
    words, _ = dedupe(qu, tokenize(qu, setup.min_word_size))
    if len(qu) > MAX_QUERY_CHARS or len(words) > MAX_QUERY_WORDS:
        return None
    return words


def match(qu, qwords, du, uniq, setup):
    """The four matchers over the query words and the document's distinct words: per query word None or a record
    dict(kind, dist, w, w2, rel, ml) — document word(s) as indices into uniq, the covered part relative to the word's start."""
    Q = [qu[o:o + l] for o, l in qwords]; D = [du[o:o + l] for o, l in uniq]
    nq, nd = len(Q), len(D)
    qa = [True] * nq; da = [True] * nd
    rec = [None] * nq; matched = [0.0] * nq

    def take(i, kind, dist, w, w2, rel, ml, ms):
        rec[i] = dict(kind=kind, dist=dist, w=w, w2=w2, rel=rel, ml=ml); matched[i] += ms; qa[i] = False

    if setup.cover_whole_words:                                            # site 1
        for i in range(nq):
            for j in range(nd):
                if da[j] and eq(Q[i], D[j]):
                    take(i, "whole", 0, j, None, 0, len(Q[i]), len(Q[i])); da[j] = False
                    break
    if setup.cover_joined_words:
        for i in range(nq - 1):                                            # site 2: two query words are one document word
            if not qa[i] or not qa[i + 1]:
                continue
            nxt = next((k for k in range(i + 1, nq) if qa[k]), -1)
            if nxt < 0:
                break
            for j in range(nd):
                if da[j] and len(D[j]) == len(Q[i]) + len(Q[nxt]) and starts(D[j], Q[i]) and ends(D[j], Q[nxt]):
                    take(i, "joined_query", 0, j, None, 0, len(Q[i]), len(Q[i])); take(nxt, "joined_query", 0, j, None, len(Q[i]), len(Q[nxt]), len(Q[nxt]))
                    da[j] = False
                    break
        for i in range(nd - 1):                                            # site 3: one query word is two consecutive document words
            if not da[i]:
                continue
            nxt = next((k for k in range(i + 1, nd) if da[k]), -1)
            if nxt < 0:
                break
            for j in range(nq):
                if qa[j] and len(Q[j]) == len(D[i]) + len(D[nxt]) and starts(Q[j], D[i]) and ends(Q[j], D[nxt]):
                    take(j, "joined_doc", 0, i, nxt, 0, len(D[i]), len(Q[j])); da[i] = False; da[nxt] = False
                    break
    if setup.cover_prefix_suffix:
        def by_length(idx, length):      # the reference's insertion sort: descending length, stable
            out = []
            for x in idx:
                k = len(out)
                while k > 0 and length(out[k - 1]) < length(x):
                    k -= 1
                out.insert(k, x)
            return out
        qi = by_length([i for i in range(nq) if qa[i]], lambda i: len(Q[i]))
        di = by_length([j for j in range(nd) if da[j]], lambda j: len(D[j]))
        for i in qi:                                                       # site 4: MatchExact
            if not qa[i]:
                continue
            ql = len(Q[i])
            for j in di:
                if not da[j]:
                    continue
                dl = len(D[j])
                if ql == dl:
                    continue
                hit = None
                if ql < dl:
                    if starts(D[j], Q[i]):
                        hit = ("prefix", 0, ql, float(ql))
                    elif ends(D[j], Q[i]):
                        hit = ("suffix", dl - ql, ql, float(max(1, ql // 2)))
                    elif ql >= 4 and index_of(D[j], Q[i]) >= 0:
                        hit = ("infix", index_of(D[j], Q[i]), ql, ql * 0.6)
                elif ends(Q[i], D[j]):
                    hit = ("tail", 0, dl, float(dl))
                if hit:
                    take(i, hit[0], 0, j, None, hit[1], hit[2], hit[3]); da[j] = False
                    break
        for i in qi:                                                       # site 5: MatchFuzzyPrefix
            if not qa[i]:
                continue
            ql = len(Q[i])
            if not (ql >= 4 or (i == nq - 1 and ql >= 2)):
                continue
            for j in di:
                if not da[j]:
                    continue
                dl = len(D[j])
                if ql >= dl:
                    continue
                hit = None
                dist = min(2, damerau(Q[i], D[j][:ql], 1))
                if dist <= 1:
                    hit = (ql, max(ql - dist, 0.1))
                elif dl > ql:
                    dist = min(2, damerau(Q[i], D[j][:ql + 1], 1))
                    if dist <= 1:
                        hit = (ql + 1, max(ql - dist, 0.1))
                    elif ql > 1:
                        dist = min(2, damerau(Q[i], D[j][:ql - 1], 1))
                        if dist <= 1:
                            hit = (ql - 1, max(ql - 1 - dist, 0.1))
                if hit:
                    take(i, "fuzzy_prefix", dist, j, None, 0, hit[0], hit[1]); da[j] = False
                    break
    if setup.cover_fuzzy_words:                                            # site 6
        f32 = np.float32
        all_full = all(not (len(Q[i]) > 0 and f32(matched[i]) < f32(len(Q[i]))) for i in range(nq))
        max_ql = max([len(Q[i]) for i in range(nq) if qa[i]] or [0])
        if not all_full and max_ql:
            def typos(ql):
                return 2 if ql >= setup.min_len_two_typos else (1 if ql >= setup.min_len_one_typo else 0)
            max_ed = typos(max_ql)
            if max_ql == 2 and max_ed == 0 and setup.num_typos >= 1:
                max_ed = 1
            max_ed = min(max_ed, setup.num_typos)
            for ed in range(1, max_ed + 1):
                if not any(qa):
                    break
                for i in range(nq):
                    if not qa[i]:
                        continue
                    ql = len(Q[i])
                    if ql < setup.min_word_size:
                        continue
                    tme = typos(ql); special = False
                    if ql == 2 and tme == 0 and setup.num_typos >= 1:
                        tme = 1; special = True
                    tme = min(tme, setup.num_typos)
                    if ed > tme or (special and ed != 1):
                        continue
                    min_len = max(setup.min_word_size, ql - ed); max_len = min(setup.lev_max_word_size, ql + ed, 63)
                    for j in range(nd):
                        if not da[j]:
                            continue
                        dl = len(D[j])
                        if dl > max_len or dl < min_len:
                            continue
                        if special and (dl == 0 or D[j][0] != Q[i][0]):
                            continue
                        dist = damerau(Q[i], D[j], ed)
                        if dist <= ed:
                            take(i, "fuzzy", dist, j, None, 0, dl, ql - dist); da[j] = False
                            break
    return rec


def span_walk(raw, which, term_of, rel, ml):
    """highlight.h hl_span_walk: (offset, length, match_offset, match_length, term) of every occurrence of a matched word, the first 64, and `truncated`."""
    spans = []
    for (off, ln), u in zip(raw, which):
        t = term_of[u]
        if t is None:
            continue
        if len(spans) == MAX_SPANS:
            return spans, True
        spans.append((off, ln, off, ln, t) if ml[t] is None else (off, ln, off + rel[t], ml[t], t))
    return spans, False


def window(raw, spans, width):
    """highlight.h hl_window, THE WINDOW RULE: (start, length)."""
    if not raw:
        return 0, 0
    best = None
    for a in ([s[0] for s in spans] or [raw[0][0]]):
        ends_ = [o + l for o, l in raw if o >= a and o + l - a <= width]
        e = max(ends_) if ends_ else a + width
        inside = [s for s in spans if a <= s[0] < e]
        rank = (len(set(s[4] for s in inside)), len(inside))
        if best is None or rank > best[0]:
            best = (rank, a, e)
    _, a, e = best
    budget = max(width - (e - a), 0) // 4
    b = min([o for o, _ in raw if o < a and a - o <= budget] or [a])
    return b, e - b


def highlight(query, doc, chars=160, setup=None):
    """What Query.highlight returns for one (query text, stored text) pair: a dict with the fields of Highlight; terms are dicts with the fields of TermMatch."""
    setup = setup or Setup()
    qu, du = units(query), units(doc)
    out = dict(status="ok", terms=[], spans=[], truncated=False, snippet="", snippet_start=0, words=0)
    qwords = query_words(qu, setup)
    if qwords is None:
        out["status"] = "long_query"
        return out
    raw = tokenize(du, setup.min_word_size)
    if len(raw) > MAX_DOC_WORDS:
        out["status"] = "too_long"
        return out
    out["words"] = len(raw)
    uniq, which = dedupe(du, raw)
    rec = match(qu, qwords, du, uniq, setup)
    term_of = [None] * len(uniq); rel = [0] * len(qwords); ml = [None] * len(qwords)
    for i, ((qo, qlen), r) in enumerate(zip(qwords, rec)):
        t = dict(word=text_of(qu[qo:qo + qlen]), kind="none", offset=0, length=0, match_offset=0, match_length=0, distance=0, offset2=0, length2=0)
        if r is not None:
            o, l = uniq[r["w"]]
            t.update(kind=r["kind"], offset=o, length=l, match_offset=o + r["rel"], match_length=r["ml"], distance=r["dist"])
            if term_of[r["w"]] is None:
                term_of[r["w"]] = i
            if r["kind"] == "joined_doc":
                t.update(offset2=uniq[r["w2"]][0], length2=uniq[r["w2"]][1])
                if term_of[r["w2"]] is None:
                    term_of[r["w2"]] = i
            if r["kind"] in ("prefix", "suffix", "infix", "fuzzy_prefix"):       # the others cover every occurrence whole
                rel[i] = r["rel"]; ml[i] = r["ml"]
        out["terms"].append(t)
    out["spans"], out["truncated"] = span_walk(raw, which, term_of, rel, ml)
    start, ln = window(raw, out["spans"], chars)
    ln = min(ln, chars, len(du) - min(start, len(du)))
    out["snippet_start"] = start; out["snippet"] = text_of(du[start:start + ln])
    return out


def _get(t, name):
    return t[name] if isinstance(t, dict) else getattr(t, name)


def features(terms, words):
    """The Stage-2 coverage features (FEATURES) that a row's term records and its document's word count determine, as k_stage2 computes them."""
    f32 = np.float32
    n = len(terms)
    matched = []; has_prefix = []; strict = []; pos = []; qlen = []
    for t in terms:
        kind = _get(t, "kind"); ql = len(units(_get(t, "word"))); dist = _get(t, "distance"); mlen = _get(t, "match_length")
        ms = {"none": 0.0, "whole": float(ql), "joined_query": float(ql), "joined_doc": float(ql), "prefix": float(ql), "suffix": float(max(1, ql // 2)),
              "infix": ql * 0.6, "tail": float(_get(t, "length")), "fuzzy": float(ql - dist),
              "fuzzy_prefix": max(float((ql - 1 if mlen == ql - 1 else ql) - dist), 0.1)}[kind]
        matched.append(f32(ms)); qlen.append(ql)
        first_of_pair = kind == "joined_query" and _get(t, "match_offset") == _get(t, "offset")
        has_prefix.append(kind in ("whole", "joined_doc", "prefix") or first_of_pair)
        strict.append(kind in ("whole", "joined_query", "joined_doc"))
        pos.append(_get(t, "offset") if kind != "none" else -1)
    full = [matched[i] >= f32(qlen[i]) - f32(0.01) for i in range(n)]
    anym = [matched[i] > 0 for i in range(n)]
    ph = [has_prefix[i] and qlen[i] > 0 and matched[i] > 0 for i in range(n)]
    hit = [p for p in pos if p >= 0]
    run = best = 0
    for x in ph:
        run = run + 1 if x else 0; best = max(best, run)
    srun = 0
    for x in reversed(ph):
        if not x:
            break
        srun += 1
    return {"WordHits": sum(1 for t in terms if _get(t, "kind") != "none"), "TermsWithAnyMatch": sum(anym), "TermsFullyMatched": sum(full),
            "TermsStrictMatched": sum(1 for i in range(n) if strict[i] and full[i]), "TermsPrefixMatched": sum(has_prefix),
            "FirstMatchIndex": min(hit) if hit else -1, "PhraseSpan": max(hit) - min(hit) + 1 if hit and sum(anym) >= 2 else 0,
            "LongestPrefixRun": best, "SuffixPrefixRun": srun,
            "PrecedingStrictCount": sum(1 for i in range(n - 1) if strict[i] and full[i]) if n >= 2 else 0, "DocTokenCount": words}
