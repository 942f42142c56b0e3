"""The exact Stage-1 replay as plain code: numpy and Python only, nothing of infidex_amd/csrc or of the oracle's sources.

replay() follows Bm25Scorer.Search as oracle/stage1.hpp:303-414 reads it, on the CSR arrays and the Term / Index / Plan objects of tests/stage1_model.py, with the
candidates of Plan.cand.  Every value is an np.float32 and every operation is rounded once (numpy's float32 arithmetic; no float64 intermediate):
  candidates    ascending doc id, grouped by doc >> 16 (one Roaring container), chunks of at most 4096 inside a group;
  terms         in scorer order; suffix sums of maxScore in fp32 from the last term backwards; a term with idf <= 0 is skipped;
  skip          per (chunk, term): a candidate is left out when (cur + maxScore) + suffix[t + 1] <= threshold, the threshold being what the chunks before left;
  formulas      the matches that remain are counted in candidate order: the first mc - mc % 8 take the eight-lane K1 * ((1 - B) + (B / avgdl) * dl), the rest
                ComputeTermScore's K1 * (1 - B + B * (dl / avgdl)) with its dl <= 0 -> 1; a virtual term has tf 1;
  heap          after a chunk every candidate with a score > 0 that is not deleted goes through UpdateTopK in doc order (a deleted one was scored with its chunk and
                shifted the positions of the others); PriorityQueue<int, float> is an array-backed 4-ary min-heap: Enqueue sifts up with <, EnqueueDequeue runs only
                for a score > the root and sifts down taking the FIRST minimal child, stopping at <=; the threshold is the root from the moment the heap holds depth;
  result        the heap's content, doc -> fp32 bits.
Beside the result a Replay says whether a case bites: chunks, skipped (candidate, term) pairs that held a posting, postings scored by the tail formula, evictions that
took place while at least two entries held the minimum score, arrivals refused for a score EQUAL to the threshold, and the threshold at every chunk start.

MISREADINGS are five deliberate wrong readings, switched on by name; they exist only here, so that tests/test_replay_model.py can show that the constructed index
below (PlateauIndex, plateau_batch) tells each of them from the right one.  tests/test_gpu_replay_plateaus.py holds the kernels to replay() on that index."""
import numpy as np

from tests import stage1_model as M

f32 = np.float32
MISREADINGS = ("no scalar tail", "eviction by (score, doc id)", "no MaxScore skip", "chunks not cut at containers", "deleted removed before counting")
_K1, _B, _ONE = f32(1.2), f32(0.75), f32(1)
_K1P1 = f32(_K1 + _ONE)
_MINDL = f32(_ONE - _B)
CHUNK = 4096


def max_score32(idf, avgdl):
    """VectorModel.SearchWithMaxScore's bound of a term (oracle/stage1.hpp:462-465) in fp32."""
    min_dl_norm = f32(_MINDL + f32(_B * f32(_ONE / f32(avgdl))))
    max_core = f32(f32(f32(255) * _K1P1) / f32(f32(255) + f32(_K1 * min_dl_norm)))
    return f32(f32(idf) * f32(max_core + _ONE))


def lane_scores(idf, tf, dl, avgdl):
    """The eight-lane formula on float32 arrays (or scalars): one rounding per operation."""
    tf = np.asarray(tf, f32); dl = np.asarray(dl, f32)
    norm = _K1 * (_MINDL + (_B / f32(avgdl)) * dl)
    return f32(idf) * ((tf * _K1P1) / (tf + norm) + _ONE)


def tail_scores(idf, tf, dl, avgdl):
    """ComputeTermScore on float32 arrays (or scalars)."""
    tf = np.asarray(tf, f32); dl = np.asarray(dl, f32)
    dl = np.where(dl <= 0, _ONE, dl).astype(f32)
    norm = _K1 * (_MINDL + _B * (dl / f32(avgdl)))
    return f32(idf) * ((tf * _K1P1) / (tf + norm) + _ONE)


def differing_pairs(idf, tfs, lengths, avgdl):
    """The (tf, length) pairs whose score the two formulas round differently for this idf."""
    return [(int(tf), float(dl)) for tf in tfs for dl in lengths
            if f32(lane_scores(idf, tf, dl, avgdl)).view(np.uint32) != f32(tail_scores(idf, tf, dl, avgdl)).view(np.uint32)]


class _Heap:
    """PriorityQueue<int, float> with the BCL's sift rules; p: Python floats holding fp32 values (comparisons are exact), d: doc ids."""

    def __init__(self):
        self.p, self.d = [], []

    def enqueue(self, doc, s):
        p, d = self.p, self.d
        i = len(p); p.append(s); d.append(doc)
        while i > 0:
            par = (i - 1) >> 2
            if s < p[par]:
                p[i] = p[par]; d[i] = d[par]; i = par
            else:
                break
        p[i] = s; d[i] = doc

    def enqueue_dequeue(self, doc, s):
        p, d = self.p, self.d
        n, i = len(p), 0
        while True:
            c = 4 * i + 1
            if c >= n:
                break
            mi, mp = c, p[c]
            for j in range(c + 1, min(c + 4, n)):
                if p[j] < mp:
                    mi, mp = j, p[j]
            if s <= mp:
                break
            p[i] = mp; d[i] = d[mi]; i = mi
        p[i] = s; d[i] = doc


class Replay:
    """result: doc -> fp32 bits; chunks; skipped; tail_postings; tied_evictions; equal_arrivals; thresholds (np.float32 per chunk start)."""


def candidate_tf(cand_docs, t):
    """float32 per candidate: the term's tf there, 0 where it has no posting (a virtual term: 1)."""
    out = np.zeros(len(cand_docs), f32)
    if len(t.docs):
        pos = np.minimum(np.searchsorted(t.docs, cand_docs), len(t.docs) - 1)
        has = t.docs[pos] == cand_docs
        out[has] = 1 if t.tf is None else t.tf[pos[has]].astype(f32)
    return out


def first_pass(ix, terms, cand):
    """(candidate docs, float32 scores) with EVERY match by the eight-lane formula, summed in scorer order: what the first pass leaves, and what k_select's plateau
    test reads."""
    docs = np.flatnonzero(cand)
    dl = ix.doc_len[docs]
    sc = np.zeros(len(docs), f32)
    for t in terms:
        if not t.idf > 0:
            continue
        tf = candidate_tf(docs, t)
        m = tf > 0
        sc[m] = sc[m] + lane_scores(t.idf, tf[m], dl[m], ix.avgdl)
    return docs, sc


def plateau_at_cut(ix, terms, cand, depth):
    """(rows, tied): the rows the cut is taken from (first-pass score > 0, not deleted) and whether rows of bit-equal first-pass score lie on both sides of the
    (score descending, doc ascending) cut at `depth`."""
    docs, sc = first_pass(ix, terms, cand)
    keep = (sc > 0) & ~ix.deleted[docs]
    docs, sc = docs[keep], sc[keep]
    if len(docs) <= depth:
        return len(docs), False
    order = np.lexsort((docs, -sc.astype(np.float64)))
    return len(docs), bool(sc[order[depth - 1]] == sc[order[depth]])


def replay(ix, terms, cand, depth, max_scores=None, misread=None):
    """cand: bool per document (Plan.cand).  max_scores: fp32 per term (default: max_score32 of its idf).  misread: None or one of MISREADINGS."""
    assert misread is None or misread in MISREADINGS
    docs = np.flatnonzero(cand)
    if misread == MISREADINGS[4]:
        docs = docs[~ix.deleted[docs]]
    T = len(terms)
    ms = [max_score32(t.idf, ix.avgdl) for t in terms] if max_scores is None else [f32(x) for x in max_scores]
    suffix = [f32(0)] * (T + 1)
    for i in range(T - 1, -1, -1):
        suffix[i] = f32(suffix[i + 1] + ms[i])
    tfs = [candidate_tf(docs, t) if t.idf > 0 else None for t in terms]
    dl = ix.doc_len[docs].astype(f32)
    gone = ix.deleted[docs]
    R = Replay()
    R.chunks = R.skipped = R.tail_postings = R.tied_evictions = R.equal_arrivals = 0
    R.thresholds = []
    heap = _Heap()
    threshold = f32(0)
    by_doc = misread == MISREADINGS[1]
    group = np.zeros(len(docs), np.int64) if misread == MISREADINGS[3] else docs >> 16
    starts = np.flatnonzero(np.r_[True, group[1:] != group[:-1]]).tolist() + [len(docs)]
    for g in range(len(starts) - 1):
        for a in range(starts[g], starts[g + 1], CHUNK):
            b = min(a + CHUNK, starts[g + 1])
            R.chunks += 1
            R.thresholds.append(threshold)
            cur = np.zeros(b - a, f32)
            for t in range(T):
                if tfs[t] is None:
                    continue
                has = tfs[t][a:b] > 0
                if misread != MISREADINGS[2]:
                    skip = ((cur + ms[t]) + suffix[t + 1]) <= threshold
                    R.skipped += int((has & skip).sum())
                    has &= ~skip
                m = np.flatnonzero(has)
                mc = len(m)
                if mc == 0:
                    continue
                lim = mc if misread == MISREADINGS[0] else mc - mc % 8
                tf = tfs[t][a:b][m]; dlm = dl[a:b][m]
                sc = np.empty(mc, f32)
                sc[:lim] = lane_scores(terms[t].idf, tf[:lim], dlm[:lim], ix.avgdl)
                sc[lim:] = tail_scores(terms[t].idf, tf[lim:], dlm[lim:], ix.avgdl)
                cur[m] = cur[m] + sc
                R.tail_postings += mc - lim
            offer = (cur > 0) & ~gone[a:b]
            for j in np.flatnonzero(offer).tolist():
                s = float(cur[j]); d = int(docs[a + j])
                if len(heap.p) < depth:
                    heap.enqueue(d, s)
                    if len(heap.p) == depth:
                        threshold = f32(min(heap.p) if by_doc else heap.p[0])
                elif s > threshold:
                    if heap.p.count(float(threshold)) >= 2:
                        R.tied_evictions += 1
                    if by_doc:      # the misreading: the (score, doc id) cut — of the entries at the minimum the largest doc id goes
                        th = float(threshold)
                        k = max((i for i in range(depth) if heap.p[i] == th), key=lambda i: heap.d[i])
                        heap.p[k] = s; heap.d[k] = d
                        threshold = f32(min(heap.p))
                    else:
                        heap.enqueue_dequeue(d, s)
                        threshold = f32(heap.p[0])
                elif s == threshold:
                    R.equal_arrivals += 1
    R.result = {d: int(f32(p).view(np.uint32)) for d, p in zip(heap.d, heap.p)}
    return R


# ---- the constructed index of tests/test_gpu_replay_plateaus.py ----------------------------------------------------------------------------------------------------
DEPTHS = (1, 2, 63, 64, 65, 500, 512, 513, 1024)
TFS = (1, 2, 3, 7, 255)
C1, C2 = 65536, 131072                                   # the first ids of containers 1 and 2
STEPS = (10, 100, 600, 600, 300, 300, 300, 300)          # rows per score step, best first: every cut of DEPTHS (ranks depth, depth + 1) lies inside one step
STEP_COMBOS = ((255, 0), (7, 0), (3, 0), (2, 0), (1, 0), (1, 1), (1, 2), (1, 3))   # (tf, length class), best first whatever the four lengths (shorter and more = better)
RISE0, FALL0 = 30000, 34000
TAIL_PER_CHUNK = (3, 8, 9, 10, 11, 12, 13, 14)           # TAIL's matches in the eight chunks of the pure zone; 7 in container 1, 15 in container 2: every residue mod 8
NESTED3, NESTED_WIDE, N_WIDE = 10000, 12000, 70
REFA_DOCS = (5, 2003)                                    # REFA's documents in containers 0 and 1: fewer than eight (all by the tail formula), and 3 mod 8
TINY_BOUND = 1e-9                                        # the maxScore handed over for REFB in "refused interval"


class PlateauIndex:
    """2 * 65 536 + 9 000 documents whose lengths take four values, so that ties are structural:
         [0, 30000) and container 2   the shortest length (class 0): the pure plateaus and the container-population lists
         [30000, 38000)               the rising and the falling staircase (STEPS rows per (tf, length class) of STEP_COMBOS, in doc order upward / downward)
         [38000, 65536)               class d % 4;    container 1: class (d >> 3) % 4
    The four lengths are the first of a fixed pseudo-random sequence for which, with the average they give, the two formulas round (tf, shortest length) differently
    for TAIL's idf at some tf >= 2 and the same at another length: picked by the model, asserted by tests/test_replay_model.py.  tf bytes: 1, 2, 3, 7, 255."""

    def __init__(self):
        N = self.N = 2 * 65536 + 9000
        d = np.arange(N, dtype=np.int64)
        cls = np.zeros(N, np.int64)
        cls[38000:C1] = d[38000:C1] % 4
        cls[C1:C2] = (d[C1:C2] >> 3) % 4
        L = {}                                             # name -> (docs, tf)
        one = lambda docs: (np.asarray(docs, np.int64), np.ones(len(docs), np.uint8))
        rng = lambda a, n: d[a:a + n]
        # staircases: rising = worst step first in doc order, falling = best step first
        for name, base, order in (("RISE", RISE0, range(len(STEPS) - 1, -1, -1)), ("FALL", FALL0, range(len(STEPS)))):
            tf = []; at = base
            for k in order:
                n = STEPS[k] + (8 if name == "FALL" and k == len(STEPS) - 1 else 0)          # (pairwise distinct df: the falling staircase's worst step is longer)
                cls[at:at + n] = STEP_COMBOS[k][1]; tf += [STEP_COMBOS[k][0]] * n; at += n
            L[name] = (rng(base, len(tf)), np.asarray(tf, np.uint8))
        self.cls = cls
        tail_docs = np.concatenate([CHUNK * k + 16 * np.arange(n) for k, n in enumerate(TAIL_PER_CHUNK)] + [70000 + 16 * np.arange(7), C2 + 16 * np.arange(15)])
        self._pick_lengths(len(tail_docs))
        L["TAIL"] = (tail_docs, np.full(len(tail_docs), self.tail_tf, np.uint8))
        g = np.concatenate([d[38000:C1][d[38000:C1] % 4 == 1], d[C1:118000][(d[C1:118000] >> 3) % 4 == 1]])       # RARE: one length class, beside C1 .. C3 everywhere
        gtf = np.asarray(TFS)[np.minimum((g - 38000) // 9000, 4)]; gtf[::16] = 1                                   # tf rises with the doc id; every 16th stays at 1
        L["RARE"] = (g, gtf.astype(np.uint8))
        k = self.refa_cls                                                             # REFA: one length class, at which the tail formula rounds ABOVE the lane formula
        c0 = d[38000:C1][d[38000:C1] % 4 == k][-REFA_DOCS[0]:]; c1 = d[C1:C2][(d[C1:C2] >> 3) % 4 == k][:REFA_DOCS[1]]
        L["REFA"] = (np.r_[c0, c1], np.full(sum(REFA_DOCS), self.refa_tf, np.uint8))
        L["REFB"] = (c1[-50:], np.full(50, 2, np.uint8))                              # the last 47 lane rows and the 3 tail rows of REFA's chunk in container 1
        L["PURE"] = one(rng(0, 30000))
        L["EQ"] = one(rng(100, 2992))
        L["CA"] = one(np.r_[C1 - 1, rng(C2, 4095)])                                  # containers of 1, 0 and 4095 candidates
        L["CB"] = one(np.r_[C1 - 1, C1, rng(C2, 4096)])                              # 1, 1, 4096
        L["CC"] = one(np.r_[rng(C1 - 4097, 4097), C2 - 1, rng(C2, 8193)])            # 4097, 1, 8193
        L["CD"] = one(np.r_[rng(0, 256), rng(C1, 257), rng(C2, 1024)])               # chunks of 256, 257 and 1024 candidates
        L["CE"] = one(np.r_[rng(0, 4096 + 256), rng(C1, 4096 + 257), rng(C2, 1025)])  # 4096 + 256, 4096 + 257, 1025
        L["COM1"] = one(rng(20000, 100000)); L["COM2"] = one(rng(30000, 90000)); L["COM3"] = one(rng(38000, 80000))
        L["SB"] = one(rng(0, 9000)); L["SC"] = one(rng(0, 60000)); L["SD"] = one(rng(0, 110000))
        for j, tf in enumerate((3, 7, 255)):                                         # three tf >= 3 terms in one row: the third goes through the posting lookup
            L["X%d" % j] = (rng(NESTED3, 1100 + j), np.full(1100 + j, tf, np.uint8))
        for j in range(N_WIDE):                                                      # nested lists: 1200 rows hold all of them, match counts 1200 + j (every residue)
            L["W%d" % j] = (rng(NESTED_WIDE, 1200 + j), np.full(1200 + j, TFS[j % 5], np.uint8))
        self.names = list(L)
        self.id = {n: i for i, n in enumerate(self.names)}
        self.lists = [L[n][0] for n in self.names]
        tfs = [L[n][1] for n in self.names]
        assert all(len(l) and (np.diff(l) > 0).all() and l[0] >= 0 and l[-1] < N for l in self.lists)
        self.T = len(self.lists)
        self.df = np.asarray([len(l) for l in self.lists], np.int32)
        assert len(set(self.df.tolist())) == self.T, "pairwise distinct df"
        self.post_off = np.zeros(self.T + 1, np.uint64); self.post_off[1:] = np.cumsum(self.df)
        self.post_doc = np.concatenate(self.lists).astype(np.int32)
        self.post_w = np.concatenate(tfs).astype(np.uint8)
        assert set(np.unique(self.post_w).tolist()) == set(TFS)
        self.idf = [M.idf32(N, len(l)) for l in self.lists]
        self.virtual = np.r_[rng(5000, 2000), rng(C2, 500)]                           # the doc set of the virtual term: 2000 rows beside PURE, 500 alone
        # deletions: inside plateaus, beside chunk and container boundaries, one of TAIL's matches, inside the nested lists and the staircases' best steps
        self.gone = np.asarray(sorted({3, 4095, 4096, 4097, 8191, 3 * CHUNK + 16, NESTED3 + 5, NESTED_WIDE + 7, RISE0 + 3, RISE0 + sum(STEPS) - 2, FALL0 + 2, 50001,
                                       C1 - 1, C1, 90009, C2 - 1, C2, C2 + 4094, C2 + 4095, C2 + 8192}))

    def _pick_lengths(self, tail_df):
        counts = np.bincount(self.cls, minlength=4).astype(np.float64)
        idf = M.idf32(self.N, tail_df)
        r = np.random.default_rng(20241)
        for _ in range(4000):
            lv = np.sort(r.choice(np.arange(3, 60), 4, replace=False)).astype(np.float64)
            avgdl = f32((counts * lv).sum() / self.N)
            diff = differing_pairs(idf, TFS[1:], lv, avgdl)
            at0 = [tf for tf, dl in diff if dl == lv[0]]
            same0 = [tf for tf in TFS[1:] if tf not in at0]
            ridf = M.idf32(self.N, REFA_DOCS[0] + REFA_DOCS[1])
            above = [(k, tf) for k in (1, 2, 3) for tf in TFS if tail_scores(ridf, tf, lv[k], avgdl) > lane_scores(ridf, tf, lv[k], avgdl)]
            if at0 and same0 and above and len(differing_pairs(M.idf32(self.N, 30000), (1,), lv[1:], avgdl)) >= 1:
                self.lengths, self.avgdl, self.tail_tf, (self.refa_cls, self.refa_tf) = lv.astype(f32), avgdl, at0[0], above[0]
                self.doc_len = self.lengths[self.cls]
                return
        raise AssertionError("no four lengths found")

    def model(self, deleted=False):
        return M.Index(self.doc_len, self.avgdl, M._mask(self.N, self.gone) if deleted else None)

    def term(self, name):
        t = self.id[name]; o = self.post_off
        return M.Term(self.lists[t], self.post_w[int(o[t]):int(o[t + 1])], self.idf[t])


def plateau_batch(P, level=2):
    """The named queries: (name, term names in ascending term id, led by the virtual term or not).  level 0: at most 4 terms (one mask word); 1: plus the query of 40
    terms (two words); 2: plus the one of 70 (four words: k_mark_wide hands it to k_exact1)."""
    q = lambda name, terms, virt=False, bounds=None: dict(name=name, terms=sorted(terms, key=lambda n: P.id[n]), virt=virt, bounds=bounds or {})
    qs = [q("pure plateau", ["PURE"]), q("rising plateau", ["RISE"]), q("falling plateau", ["FALL"]),
          q("containers 1/0/4095", ["CA"]), q("containers 1/1/4096", ["CB"]), q("containers 4097/1/8193", ["CC"]),
          q("chunks 256/257/1024", ["CD"]), q("chunks 4096+256/4096+257/1025", ["CE"]),
          q("tails 0..7", ["TAIL", "PURE"]), q("maxscore skips", ["RARE", "COM1", "COM2", "COM3"]), q("arrival equals threshold", ["EQ"]),
          q("3 terms tf>=3", ["X0", "X1", "X2"]), q("virtual term", ["PURE"], virt=True), q("100 x depth stop", ["SB", "SC", "SD"]),
          # At depths 1 and 2 the heap is full after container 0, whose five rows all took the tail formula: the exact threshold lies one ulp ABOVE the one
          # predicted from first-pass scores.  The maxScore handed over for REFB is deliberately no bound at all (the replay follows the reference whatever it
          # is given): cur + maxScore is then cur itself, at REFB's turn the predicted threshold skips the lane rows only, the exact one the tail rows too,
          # and a kernel that took the predicted decisions would let the tail rows, REFB's score added, into the heap.  k_ex_heap has to refuse the interval.
          q("refused interval", ["REFA", "REFB"], bounds={"REFB": TINY_BOUND})]
    if level >= 1:
        qs.append(q("40 terms", ["W%d" % j for j in range(40)]))
    if level >= 2:
        qs.append(q("70 terms", ["W%d" % j for j in range(N_WIDE)]))
    return qs


def plateau_model(P, Q, depth, deleted=False):
    """(Index, terms in scorer order, Plan, fp32 maxScore per term) of one query of plateau_batch at one depth.  The mode is the batch's (disjunctive: the ABI takes
    it from the host); a maxScore is max_score32 of the term's idf unless the query says otherwise."""
    ix = P.model(deleted)
    terms = [M.Term(P.virtual, None, M.idf32(P.N, len(P.virtual)))] if Q["virt"] else []      # fuzzy virtual terms come first (VectorModel.cs:442)
    terms += [P.term(n) for n in Q["terms"]]
    ms = [max_score32(t.idf, ix.avgdl) for t in terms]
    for n, v in Q["bounds"].items():
        ms[Q["terms"].index(n) + len(terms) - len(Q["terms"])] = f32(v)
    return ix, terms, M.plan(ix, terms, depth, [], mode=M.MODE_DISJ), ms


# ---- the tie corpus of tests/test_replay_model.py and tests/test_gpu_replay_plateaus.py ------------------------------------------------------------------------------
TIE_DOCS = 140000                                          # more than 131 072: two container boundaries are crossed
TIE_DEPTHS = (1, 7, 64, 500)
TIE_WORDS = ("amber", "birch", "cedar", "delta", "ember", "flint", "grove", "heron", "ivory", "jolly", "koala", "lemon",
             "maple", "noble", "ocean", "pearl", "quilt", "river", "stone", "tulip", "umbra", "viola", "wheat", "zebra")


def tie_corpus():
    """(texts of TIE_DOCS short documents, [(query text, depth)]): the documents are drawn from 40 templates of two to six words over TIE_WORDS, the common templates
    thousands of times, so thousands of documents share their length and every matched term; the queries are single words and runs of two or three words of a common template."""
    r = np.random.default_rng(9)
    templates = [" ".join(r.choice(TIE_WORDS, int(r.integers(2, 7)))) for _ in range(40)]
    w = 1.0 / (1.0 + np.arange(40)); w /= w.sum()
    pick = r.choice(40, TIE_DOCS, p=w)
    texts = [templates[k] for k in pick]
    queries = []
    for depth in TIE_DEPTHS:                                # eleven single words and four runs of two or three words of one of the six commonest templates (their documents are many)
        for w1 in r.choice(TIE_WORDS, 11, replace=False):
            queries.append((str(w1), depth))
        for k in r.choice(6, 4, replace=False):
            ws = templates[k].split(); n = min(len(ws), int(r.integers(2, 4))); a = int(r.integers(0, len(ws) - n + 1))
            queries.append((" ".join(ws[a:a + n]), depth))
    return texts, queries
