"""The Stage-1 cut (k_rules / k_select with k_select_order and k_selg_hist / k_selg_cut / k_selg_gather) as plain code: numpy and Python only, nothing of infidex_amd/csrc.

The rows of a query are the candidates that pass the tier rule, hold a first-pass fp32 score > 0 and are not deleted.  The first pass is replay_model.first_pass — one
rounded fp32 operation per step, every match by the eight-lane formula, terms summed in scorer order — so the score BITS of every row are known here, and the cut is a
total order: score bits descending, doc id ascending.  cut() returns the first `depth` rows in that order, the hit count, `next` (the fp32 score of the best row left
out, 0 when nothing is left out) and the replay flag: with c the score of the last row taken, flagged when next > 0 and next >= f32(c * f32(f32(1) - f32(1e-5))); why 0
when next == c, else 1.

The tier rule is read from the class counts (rule_of): the disjunctive walk of TieredCandidateSelector as stage1_model.plan reads it — ranks in idf-descending order, a
low-quality rank skipped once a selective one produced a document, the stop at 100 * depth — gives the cutoff rank; Tier 0 / 1 / 2 of the AND mode give the class mask;
prefix precedence lets every row through.  `total` is what the kernels take as the number of rows the rule lets through (deleted documents included; + 128 in the
disjunctive mode for pre-"seen" documents, which the histogram does not count): it decides take-all.

path_of() documents the fixture — it is no correctness check.  From the model's score bits and the geometry DESIGN.md section 4 describes (origin M = the best score of
all emitted live rows, rejected classes included; 4095 bins of 2^12 score bits below M; sort capacity 2048; coarse bins of 2^16; partitions of max(16384, rows / 32))
it names the path a query is built to take: "take-all", "mode 1", "mode 2", "mode 3" (replay on) or "radix" (replay off), "second attempt", "radix after a missed
window", and for swept queries "swept fine", "swept coarse", "swept take-all", "swept refused"; for the radix path also the last digit reached (shift 52, 40, 28, 16, 4).

UNREACHABLE, shown by the model: the radix select's final 4-bit pass at shift 0.  After the pass at shift 4 the undecided keys agree in bits 4 .. 63, so they are at most 16
(doc ids are distinct); the loop goes on only while rows already taken + undecided > 2048, and rows already taken < depth <= 1024 (INFX_POST_MAX_ROWS, the largest
max_depth): 1023 + 16 < 2048.  path_of asserts it never gets there.  Also unreachable: a "mode 2" whose cut falls on the LAST low-bit value present in its bin — nothing of
the bin is then left out, the rows down to the bin are more than the sort holds (else it were mode 1), and the query is mode 3 / radix.  The batch has the latest value that
can be reached instead (depth 1024 in a bin of thousands).

MISREADINGS are four deliberate wrong readings of the cut, switched on by name; they exist only here, so that tests/test_select_model.py can show that the constructed
index below (SelectIndex, select_batch) tells each of them from the right one.  tests/test_gpu_select_cuts.py holds the kernels to cut() on that index."""
import numpy as np

from tests import stage1_model as M
from tests import replay_model as RM

f32, u32 = np.float32, np.uint32
SEL_CAP = 2048                     # rows the LDS sort holds
BINS, FINE, COARSE = 4095, 12, 16  # bins below the origin; log2 of the fine and the coarse bin width in score bits
PART_MIN, PARTS = 16384, 32
ORDER_MIN, ORDER_MAX = 64, 4096    # batch sizes between which k_select_order (and with it the sweeps) runs
GIANT_DEFAULT = 65536
MAX_DEPTH = 1024
MISREADINGS = ("ties cut by descending doc id", "band compared with >", "next from the cut's bin only", "rejected rows ignored for the window")
PATHS = ("take-all", "mode 1", "mode 2", "mode 3", "radix", "second attempt", "radix after a missed window",
         "swept fine", "swept coarse", "swept take-all", "swept refused")


def bits(x):
    return np.asarray(x, f32).view(u32)


def band_edge(c):
    """The lowest fp32 score of a left-out row that still flags a cut at score c."""
    return f32(f32(c) * f32(f32(1) - f32(1e-5)))


class Cut:
    """docs, bits (the rows taken, in order), hits, next (np.float32), flagged, why (None when not flagged)."""


def cut(docs, sbits, depth, origin=None, total=None, misread=None):
    """docs / sbits: the rows (passing the rule, score > 0, not deleted), any order.  origin (score bits of the best emitted live row) and total (the rule's) are read
    by two of the misreadings only."""
    assert misread is None or misread in MISREADINGS
    docs = np.asarray(docs, np.int64); sbits = np.asarray(sbits, u32)
    if misread == MISREADINGS[3] and total is not None and total > SEL_CAP and len(docs):      # one window below the origin and no second look: rows outside it are lost
        keep = ((np.int64(origin) - sbits.astype(np.int64)) >> FINE) < BINS
        docs, sbits = docs[keep], sbits[keep]
    order = np.lexsort((-docs if misread == MISREADINGS[0] else docs, -sbits.astype(np.int64)))
    docs, sbits = docs[order], sbits[order]
    C = Cut()
    C.docs, C.bits, C.hits = docs[:depth], sbits[:depth], int(min(depth, len(docs)))
    C.next = f32(0)
    if len(docs) > depth:
        C.next = sbits[depth:depth + 1].view(f32)[0]
        if misread == MISREADINGS[2]:
            o = np.int64(sbits[0] if origin is None else origin)
            same = ((o - np.int64(sbits[depth])) >> FINE) == ((o - np.int64(sbits[depth - 1])) >> FINE)
            if not same:
                C.next = f32(0)
    C.flagged, C.why = False, None
    if C.next > 0:
        c = sbits[depth - 1:depth].view(f32)[0]
        C.flagged = bool(C.next > band_edge(c)) if misread == MISREADINGS[1] else bool(C.next >= band_edge(c))
        if C.flagged:
            C.why = 0 if C.next == c else 1
    return C


class Rule:
    """passes (bool per class byte 0 .. 255), total, cutoff (DISJ) or mask (AND)."""


def rule_of(mode, counts, depth, n_and, df_s1, df_s2):
    """The tier rule from the 136 class counts.  A class byte is the lowest rank of a generating term that hit (DISJ; bit 7: a pre-"seen" document), the bits
    Tier 0 | Tier 1 | S1 | S2 (AND), 1 (PREFIX)."""
    c = [int(x) for x in counts]
    k = int(depth)
    R = Rule(); R.cutoff = R.mask = None
    cls = np.arange(256)
    if mode == M.MODE_PREFIX:
        R.passes = np.ones(256, bool); R.total = c[1]
        return R
    if mode == M.MODE_DISJ:
        # plan(): ranks [0, n_and) are not low-quality; `local` counts documents new at their lowest rank; a low-quality rank is walked only while no selective one has produced a document
        n_ranks = max(df_s1, max((i + 1 for i in range(128) if c[i]), default=0))
        has_sel, local, cutoff = False, 0, -1
        for r in range(n_ranks):
            lowq = r >= n_and
            if n_ranks > 1 and lowq and has_sel:
                continue
            cutoff = r; local += c[r]
            if not lowq and local > 0:
                has_sel = True
            if local >= k * 100:
                break
        R.cutoff = cutoff
        R.passes = (cls & 0x7F) <= cutoff
        R.total = sum(c[:cutoff + 1]) + 128
        return R
    assert mode == M.MODE_AND
    t0 = sum(c[i] for i in range(16) if i & 1)            # documents holding every term
    t1 = sum(c[i] for i in range(16) if i & 2)            # ... every term but the lowest-idf one (counted from three terms on)
    if t0 >= 2 * k:
        mask = 1
    else:
        g, mask = t0, 1
        if n_and >= 3 and t0 < 3 * k:
            g, mask = t1, 3
        if g < 5 * k and df_s1 > 0:                       # Tier 2: the most selective term's documents, and the second's unless the first alone reaches 10 * depth
            mask |= 4                                     # (G is a subset of S1: |G u S1| = df_s1)
            if df_s1 < 10 * k and df_s2 > 0:
                mask |= 8
    R.mask = mask
    R.passes = (cls & mask) != 0
    R.total = sum(c[i] for i in range(16) if i & mask)
    return R


def doc_classes(ix, terms, P):
    """(emit, cls): which documents k_accumulate emits a row for when their score is > 0, and the class byte of each."""
    N = ix.N
    cls = np.zeros(N, np.int64)
    if P.mode == M.MODE_PREFIX:
        return P.cand.copy(), cls + 1
    if P.mode == M.MODE_DISJ:
        mr = np.full(N, 999, np.int64)
        for t, role, rank in zip(terms, P.roles, P.ranks):
            if role & (M.ROLE_ELIGIBLE | M.ROLE_LOWQ):
                mr[t.docs] = np.minimum(mr[t.docs], rank)
        emit = mr < 999
        cls[emit] = mr[emit] & 0x7F
        if P.preseen is not None:
            cls[emit & P.preseen] |= 0x80
        return emit, cls
    hits = np.zeros(N, np.int64); low = np.zeros(N, bool); s1 = np.zeros(N, bool); s2 = np.zeros(N, bool)
    for t, role in zip(terms, P.roles):
        if role & M.ROLE_AND: hits[t.docs] += 1
        if role & M.ROLE_LOWEST: low[t.docs] = True
        if role & M.ROLE_S1: s1[t.docs] = True
        if role & M.ROLE_S2: s2[t.docs] = True
    t1 = hits == P.n_and - 1
    return s1 | s2, (t1 & low) * 1 + (t1 & (P.n_and >= 3)) * 2 + s1 * 4 + s2 * 8


class Sel:
    """One query on the model: ix, terms, plan, counts (136), rule, depth, docs / bits (the rows), origin (score bits of the best emitted live row), arena (rows of
    the query's arena region: every document a generating list or the DocSet names, emitted or not), max_scores."""

    def cut(self, misread=None):
        return cut(self.docs, self.bits, self.depth, self.origin, self.rule.total, misread)


def select(ix, terms, depth, mode, pset=None):
    S = Sel()
    S.ix, S.terms, S.depth = ix, terms, int(depth)
    P = S.plan = M.plan(ix, terms, depth, [] if pset is None else [pset], mode=mode)
    emit, cls = doc_classes(ix, terms, P)
    docs, sc = RM.first_pass(ix, terms, emit)
    pos = sc > 0
    S.counts = np.zeros(M.NCLASS, u32)
    counted = pos & (cls[docs] < 0x80)
    S.counts[:128] = np.bincount(cls[docs][counted], minlength=128)[:128]
    S.rule = rule_of(P.mode, S.counts, depth, P.n_and, P.df_s1, P.df_s2)
    live = pos & ~ix.deleted[docs]
    S.origin = int(bits(sc[live]).max()) if live.any() else 0
    keep = live & S.rule.passes[cls[docs]]
    S.docs, S.bits = docs[keep], bits(sc[keep]).copy()
    gen = np.zeros(ix.N, bool)
    if P.mode == M.MODE_PREFIX:
        gen = P.cand
    else:
        for t in terms:
            gen[t.docs] = True
    S.arena = int(gen.sum())
    S.max_scores = [RM.max_score32(t.idf, ix.avgdl) for t in terms]
    return S


def _find_bin(hist_bins, want):
    """k_select's find_bin on the bin number of every counted row: (bin, rows before it, rows in it), bin None when the count never reaches `want`."""
    if len(hist_bins) < want:
        return None, len(hist_bins), 0
    b = np.sort(hist_bins)
    sel = int(b[want - 1])
    return sel, int((b < sel).sum()), int((b == sel).sum())


def _radix(docs, sbits, depth, total):
    """The general radix select on the 64-bit key (score bits << 32) | ~doc: the shifts of the passes it makes."""
    keys = (sbits.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - docs.astype(np.uint64))
    und = np.ones(len(keys), bool)
    remain, undecided, shift, width, passes = depth, total, 52, 12, []
    while depth - remain + undecided > SEL_CAP and shift >= 0:
        passes.append(shift)
        digit = ((keys >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)
        d = np.sort(digit[und])[::-1]
        sel = int(d[min(remain, len(d)) - 1])
        remain -= int((digit[und] > sel).sum())
        und &= digit == sel
        undecided = int(und.sum())
        shift, width = (0, 4) if shift == 4 else (-1, width) if shift == 0 else (shift - 12, 12)
    assert 0 not in passes, "the 4-bit pass at shift 0 was reached"
    return passes


def path_of(S, replay, giant_min=0, nq=1, lpt=True, batch_bound=0):
    """(path, last radix shift or None) of the query under: the replay on or off, INFX_SEL_GIANT_MIN, the batch's query count, INFX_SELECT_LPT, and the largest row
    bound of a query of the batch (the sweeps are launched only when it reaches 4 * giant_min)."""
    depth, total = S.depth, S.rule.total
    sb = S.bits.astype(np.int64)
    swept = lpt and ORDER_MIN <= nq <= ORDER_MAX and giant_min > 0 and batch_bound >= 4 * giant_min and S.arena >= giant_min
    pre = ""
    if swept:
        if total <= SEL_CAP:
            return "swept take-all", None
        for shift, name in ((FINE, "swept fine"), (COARSE, "swept coarse")):
            b, above, und = _find_bin(((S.origin - sb) >> shift)[((S.origin - sb) >> shift) < BINS], depth)
            if b is not None and above + und <= SEL_CAP:
                return name, None
        pre = "swept refused"
    if total <= SEL_CAP:
        return "take-all", None
    origin, second = S.origin, False
    b = (origin - sb) >> FINE
    b1, above1, und1 = _find_bin(b[b < BINS], depth)
    if b1 is None:
        origin, second = int(sb.max()) if len(sb) else 0, True
        b = (origin - sb) >> FINE
        b1, above1, und1 = _find_bin(b[b < BINS], depth)
        if b1 is None:
            return pre or "radix after a missed window", _radix(S.docs, S.bits, depth, total)[-1]
    if above1 + und1 <= SEL_CAP:
        return pre or ("second attempt" if second else "mode 1"), None
    lo = ((origin - sb) & 4095)[b == b1]
    b2, above2, und2 = _find_bin(lo, depth - above1)
    if above1 + above2 + und2 <= SEL_CAP:
        return pre or ("second attempt" if second else "mode 2"), None
    if replay:
        return pre or "mode 3", None
    return pre or "radix", _radix(S.docs, S.bits, depth, total)[-1]


# ---- the constructed index of tests/test_gpu_select_cuts.py ----------------------------------------------------------------------------------------------------------
N_DOCS = 70001                    # a second 65 536-id container exists
AVGDL = 300.0
A0, A_N = 0, 40000                # lengths 40 + i / 64: every score its own
P1_0, P1_N = 41000, 3100          # a plateau inside one block of 65 536 ids (length 25, tf 3)
P3_0, P3_N = 44200, 100           # rows a little better than that plateau, inside its bin
Z0, Z_N = 44400, 100              # documents no list names: holes of a DocSet
T0, T_N = 45000, 3000             # the take-all queries' rows
PAD0, PAD_N = 48000, 64           # one-row queries
S0, S_N = 50000, 50               # short documents: the rejected rows far above the window
E0 = 52000                        # the band-edge documents
F0, F_N = 54000, 2100             # long documents: rows far below every cut
G0, G_N = 56200, 2100             # the same, all deleted by infx_set_deleted
P2_0, P2_N = 64000, 3100          # a plateau over both containers: 1536 rows in the first, 1564 in the second
EDGE_DEPTH, EDGE_IDF, EDGE_TF, EDGE_LEN = 64, 3.0, 3, 30.0


def _scan(start, down, n=3000000):
    """n successive fp32 values from `start`, upward or downward."""
    b0 = int(bits(start))
    b = np.arange(b0, b0 - n, -1, dtype=np.int64) if down else np.arange(b0, b0 + n, dtype=np.int64)
    return b.astype(u32).view(f32)


class _Base:
    def model(self, deleted=False):
        return M.Index(self.doc_len, self.avgdl, M._mask(self.N, self.gone) if deleted else None)

    def _finish(self, L):
        self.names = list(L)
        self.id = {n: i for i, n in enumerate(self.names)}
        self.lists = [np.asarray(L[n][0], np.int64) for n in self.names]
        self.tfs = [np.asarray(L[n][1], np.uint8) for n in self.names]
        assert all(len(l) and (np.diff(l) > 0).all() and l[0] >= 0 and l[-1] < self.N for l in self.lists)
        assert all(len(l) == len(t) and t.min() >= 1 for l, t in zip(self.lists, self.tfs))
        self.T = len(self.lists)
        self.df = np.asarray([len(l) for l in self.lists], np.int32)
        self.post_off = np.zeros(self.T + 1, np.uint64); self.post_off[1:] = np.cumsum(self.df)
        self.post_doc = np.concatenate(self.lists).astype(np.int32)
        self.post_w = np.concatenate(self.tfs).astype(np.uint8)

    def select(self, Q, deleted=False):
        """The Sel of one query of a batch."""
        ix = self.model(deleted)
        terms = [M.Term(self.lists[self.id[n]], self.tfs[self.id[n]], idf) for n, idf in Q["terms"]]
        return select(ix, terms, Q["depth"], Q["mode"], None if Q["pset"] is None else self.sets[Q["pset"]])


class SelectIndex(_Base):
    """70 001 documents of fp32 lengths chosen per document (avgdl 300 is handed over as it is), the lists and DocSets of select_batch's named queries."""

    def __init__(self):
        N = self.N = N_DOCS
        self.avgdl = f32(AVGDL)
        d = np.arange(N, dtype=np.int64)
        dl = np.full(N, 100.0, f32)
        dl[A0:A0 + A_N] = (40.0 + np.arange(A_N) / 64.0).astype(f32)
        dl[P1_0:P1_0 + P1_N] = 25.0
        dl[P3_0:P3_0 + P3_N] = (25.0 - (1 + np.arange(P3_N)) * 0.001).astype(f32)
        dl[T0:T0 + T_N] = (10.0 + np.arange(T_N) * 0.01).astype(f32)
        dl[PAD0:PAD0 + PAD_N] = (5.0 + np.arange(PAD_N)).astype(f32)
        dl[S0:S0 + S_N] = 1.0
        dl[F0:F0 + F_N] = (2000.0 + np.arange(F_N)).astype(f32)
        dl[G0:G0 + G_N] = (2000.0 + np.arange(G_N)).astype(f32)
        dl[P2_0:P2_0 + P2_N] = 25.0
        rng = lambda a, n: d[a:a + n]
        const = lambda docs, tf: (np.asarray(docs, np.int64), np.full(len(docs), tf, np.uint8))
        L = {}
        L["A1"] = const(rng(A0, A_N), 1)
        L["A255"] = const(rng(A0, A_N), 255)
        L["A1s"] = const(rng(A0, 2049), 1)
        L["A7a"] = const(rng(A0, 1920), 7)                         # disjunctive: 1920 + 128 = 2048 = the sort's capacity: take-all
        L["A7b"] = const(rng(A0, 1921), 7)                         # 2049: the smallest number that leaves take-all
        L["R0"] = const(rng(A0 + 1000, 3000), 1)                   # the rank-0 term of "second attempt": 100 * depth documents at depth 30
        L["HI"] = const(d[A0:A0 + A_N:700], 1)                     # 58 documents: fewer than the depth
        for j in range(20):
            L["H%d" % j] = const(rng(S0, S_N - j), 255)            # (pairwise distinct df)
        L["P1"] = const(rng(P1_0, P1_N), 3)
        L["P2"] = const(rng(P2_0, P2_N), 3)
        L["P3"] = const(np.r_[rng(P1_0, P1_N), rng(P3_0, P3_N)], 3)
        tt = rng(T0, T_N)
        L["TT"] = (tt, (1 + (tt * 7) % 255).astype(np.uint8))
        for n in (1, 2, 62, 64, 66, 499, 501, 1000, 1025):
            L["T%d" % n] = (tt[:n], (1 + (tt[:n] * 7) % 255).astype(np.uint8))
        L["ALL"] = const(d, 1)
        for j in range(PAD_N):
            L["PAD%d" % j] = const([PAD0 + j], 1 + j % 5)
        # band edge: B (62 rows better than the cut row), C (the cut row), Mg / Mn (the best row: it puts C's bin so that the edge lies in the same bin / in the next one),
        # Xe / Xb / Xq (the best row left out: on the edge, one ulp below it, equal to the cut row); lengths found by a scan over successive fp32 lengths
        sc = lambda lens: bits(RM.lane_scores(EDGE_IDF, EDGE_TF, lens, self.avgdl)).astype(np.int64)
        c = int(sc(f32(EDGE_LEN)))
        edge = int(bits(band_edge(np.asarray(c, np.int64).astype(u32).view(f32))))
        self.edge_ulps = c - edge                                  # how far below the cut the edge lies
        up = _scan(EDGE_LEN, False); s_up = sc(up)
        dn = _scan(EDGE_LEN - 1.0, True); s_dn = sc(dn)
        pick = lambda lens, s, ok: lens[np.flatnonzero(ok(s))[0]]
        lo_of = lambda s: (s - c) & 4095                           # C's low 12 bits below an origin s
        B = E0 + np.arange(62); C_, Mg, Mn, Xe, Xb, Xq = E0 + 62, E0 + 63, E0 + 64, E0 + 65, E0 + 66, E0 + 67
        dl[B] = (EDGE_LEN - 0.01 * (1 + np.arange(62))).astype(f32)
        dl[C_] = EDGE_LEN; dl[Xq] = EDGE_LEN
        dl[Xe] = pick(up, s_up, lambda s: s == edge)
        dl[Xb] = pick(up, s_up, lambda s: s == edge - 1)
        dl[Mg] = pick(dn, s_dn, lambda s: (s - c >= 4096) & (lo_of(s) >= 64) & (lo_of(s) < 2048))
        dl[Mn] = pick(dn, s_dn, lambda s: (s - c >= 4096) & (lo_of(s) >= 4096 - 32))
        self.edge_docs = dict(C=C_, Mg=Mg, Mn=Mn, Xe=Xe, Xb=Xb, Xq=Xq)
        fill = lambda docs, tail: (np.r_[docs, tail], np.r_[np.full(len(docs), EDGE_TF), np.ones(len(tail))].astype(np.uint8))
        F, G = rng(F0, F_N), rng(G0, G_N)
        for name, m, x, tail in (("Eeg", Mg, Xe, F), ("Een", Mn, Xe, F), ("Ebg", Mg, Xb, F), ("Ebn", Mn, Xb, F), ("Eqg", Mg, Xq, F), ("Ex", Mg, None, G)):
            L[name] = fill(np.sort(np.r_[B, C_, m] if x is None else np.r_[B, C_, m, x]), tail)
        self.doc_len = dl
        self._finish(L)
        # DocSets: 0 / 1 = 2048 / 2049 take-all rows (prefix precedence counts no pre-"seen" allowance: exactly the sort's capacity, and one more);
        # 2 = 501 rows and 100 documents no list names; 3 = the 40 000 spaced documents
        self.sets = [tt[:2048], tt[:2049], np.r_[rng(Z0, Z_N), tt[:501]], rng(A0, A_N)]
        self.sets[2] = np.sort(self.sets[2])
        # deletions: inside the plateaus (their first rows, rows at and beside the cut at depth 500, the container boundary), among the take-all rows, every row of G,
        # and the cut row and the best row left out of the 40 000-row query
        gone = {P1_0, P1_0 + 1, P1_0 + 499, P1_0 + 500, P1_0 + 501, P1_0 + 2999, P2_0, P2_0 + 499, P2_0 + 500, 65535, 65536, P3_0 + 3,
                T0, T0 + 61, T0 + 63, T0 + 498, T0 + 500, T0 + 2047, PAD0 + 5} | set(G.tolist())
        big = self.select(dict(terms=[("A1", 2.0)], depth=500, mode=M.MODE_DISJ, pset=None)).cut()
        gone |= {int(big.docs[-1]), int(big.docs[-2]), int(big.docs[0])}
        self.gone = np.asarray(sorted(gone))


def select_queries():
    """The named queries: name, terms ((list name, idf handed over), ascending term id), depth, mode, pset, and what each is built for: path (replay off, no sweeps),
    digit (last radix shift), path3 (replay on, where it differs), swept (the path under INFX_SEL_GIANT_MIN=64 in a batch of >= 64 queries), flag (None: not flagged;
    0 / 1: why).  All of it is asserted against path_of / cut by tests/test_select_model.py."""
    D, A, P = M.MODE_DISJ, M.MODE_AND, M.MODE_PREFIX

    def q(name, terms, depth, path, mode=D, pset=None, digit=None, path3=None, swept=None, flag=None):
        return dict(name=name, terms=terms, depth=depth, mode=mode, pset=pset, path=path, digit=digit, path3=path3 or path, swept=swept, flag=flag)
    ta = "swept take-all"
    qs = [q("take-all 1 row depth 1", [("T1", 2.0)], 1, "take-all"),
          q("take-all 1 row depth 2", [("T1", 2.0)], 2, "take-all"),
          q("take-all 2 rows depth 1", [("T2", 2.0)], 1, "take-all"),
          q("take-all depth-1 rows", [("T62", 2.0)], 63, "take-all"),
          q("take-all depth rows", [("T64", 2.0)], 64, "take-all", swept=ta),
          q("take-all depth+1 rows", [("T66", 2.0)], 65, "take-all", swept=ta),
          q("take-all 499 rows depth 500", [("T499", 2.0)], 500, "take-all", swept=ta),
          q("take-all 501 rows depth 500", [("T501", 2.0)], 500, "take-all", swept=ta),
          q("take-all 1025 rows depth 1024", [("T1025", 2.0)], 1024, "take-all", swept=ta),
          q("take-all 2048 rows prefix", [("TT", 2.0)], 64, "take-all", mode=P, pset=0, swept=ta, flag=1),
          q("take-all 1920 rows disj", [("A7a", 2.0)], 500, "take-all", swept=ta, flag=1),
          q("take-all holes and deletions", [("TT", 2.0)], 500, "take-all", mode=P, pset=2, swept=ta),
          q("mode 1 2049 rows prefix", [("TT", 2.0)], 64, "mode 1", mode=P, pset=1, swept="swept fine", flag=1),
          q("mode 1 1921 rows disj", [("A7b", 2.0)], 500, "mode 1", swept="swept fine", flag=1),
          q("mode 1 2049 rows", [("A1s", 2.0)], 500, "mode 1", swept="swept fine"),
          q("mode 1 2049 rows and", [("A1", 2.0), ("A1s", 2.5)], 500, "mode 1", mode=A, swept="swept fine"),
          q("mode 1 40000 rows", [("A1", 2.0)], 500, "mode 1", swept="swept fine"),
          q("mode 2 first value", [("A255", 2.0)], 1, "mode 2", swept="swept refused", flag=1),
          q("mode 2 depth 500", [("A255", 2.0)], 500, "mode 2", swept="swept refused", flag=1),
          q("mode 2 latest value", [("A255", 2.0)], 1024, "mode 2", swept="swept refused", flag=1),
          q("plateau one block", [("P1", 2.0)], 500, "radix", digit=4, path3="mode 3", swept="swept refused", flag=0),
          q("plateau one block depth 1024", [("P1", 2.0)], 1024, "radix", digit=4, path3="mode 3", swept="swept refused", flag=0),
          q("plateau both containers", [("P2", 2.0)], 500, "radix", digit=16, path3="mode 3", swept="swept refused", flag=0),
          q("plateau below better rows", [("P3", 2.0)], 500, "radix", digit=4, path3="mode 3", swept="swept refused", flag=0),
          q("second attempt", [("R0", 5.0)] + [("H%d" % j, 4.9 - 0.01 * j) for j in range(20)], 30, "second attempt", swept="swept coarse"),
          q("missed window", [("A1", 0.01), ("HI", 10.0)], 500, "radix after a missed window", mode=P, pset=3, digit=40, swept="swept coarse"),
          q("rejected giant", [("A1", 4.0), ("T1000", 5.0), ("ALL", 3.0)], 10, "take-all", swept=ta, flag=1),
          q("band edge gathered", [("Eeg", EDGE_IDF)], EDGE_DEPTH, "mode 1", swept="swept fine", flag=1),
          q("band edge not gathered", [("Een", EDGE_IDF)], EDGE_DEPTH, "mode 1", swept="swept fine", flag=1),
          q("band below gathered", [("Ebg", EDGE_IDF)], EDGE_DEPTH, "mode 1", swept="swept fine"),
          q("band below not gathered", [("Ebn", EDGE_IDF)], EDGE_DEPTH, "mode 1", swept="swept fine"),
          q("band equal", [("Eqg", EDGE_IDF)], EDGE_DEPTH, "mode 1", swept="swept fine", flag=0),
          q("exactly depth rows", [("Ex", EDGE_IDF)], EDGE_DEPTH, "mode 1", swept="swept fine")]
    return qs


BATCH_SIZES = (63, 64, 65, 100)


def select_batch(level):
    """The named queries padded with one-row queries to BATCH_SIZES[level] = 63 (no order kernel), 64, 65 or 100 (its bitonic sort padded to 128).  The pads all hold one
    row, several named queries hold equal row counts: the order's tie rule (lower query first) is met."""
    qs = select_queries()
    n = BATCH_SIZES[level]
    assert len(qs) < n
    for j in range(n - len(qs)):
        qs.append(dict(name="pad %d" % j, terms=[("PAD%d" % (j % PAD_N), 1.0 + j % 3)], depth=(1, 2, 63)[j % 3], mode=M.MODE_DISJ, pset=None,
                       path="take-all", digit=None, path3="take-all", swept=None, flag=None))
    return qs


def batch_bound(S, qs):
    """The largest row bound of a query of the batch: the generating lists' lengths added up (the DocSet's for prefix precedence), at most N."""
    best = 0
    for Q in qs:
        b = len(S.sets[Q["pset"]]) if Q["mode"] == M.MODE_PREFIX else sum(int(S.df[S.id[n]]) for n, _ in Q["terms"])
        best = max(best, min(b, S.N))
    return best


class TinyIndex(_Base):
    """1000 documents, one single-document list each: the batches of 4096 and 4097 one-row queries (at 4097 the order kernel is dropped)."""

    def __init__(self):
        N = self.N = 1000
        self.avgdl = f32(20.0)
        self.doc_len = (10.0 + np.arange(N) % 50).astype(f32)
        self._finish({"L%d" % i: ([i], [1 + i % 7]) for i in range(N)})
        self.sets = []
        self.gone = np.asarray([0, 7, 999])


def tiny_batch(n):
    return [dict(name="one row %d" % i, terms=[("L%d" % ((i * 7) % 1000), 1.0 + i % 5)], depth=1 + i % 2, mode=M.MODE_DISJ, pset=None) for i in range(n)]
