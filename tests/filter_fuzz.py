"""Seeded generator of Infiscript expression TREES for the filter tests (tests/test_filter_model.py on the CPU, tests/test_gpu_filter_fuzz.py on the GPU).
No tests in here.

A tree is a tuple:
    ("leaf", text)          field <op> constants, printed as is: one P_LEAF op
    ("ne", field, literal)  printed `field != lit` or `NOT (field = lit)`: the leaf `field = lit` and a NOT, two ops
    ("lit", text)           a bare literal operand: never a bool
    ("not", x)  ("and", l, r)  ("or", l, r)  ("tern", c, a, b)

text() prints a tree with only the parentheses the grammar's precedence `?: < OR < AND < NOT` requires (AND / OR are left-associative, so a right-nested
chain keeps its parentheses and a left-nested one has none); evaluate() restates the three-valued rules of the header comment of
infidex_amd/csrc/host/filter.h from the tree itself — it never sees the text, so a precedence or associativity error that the product's and the oracle's
parsers shared would show against it.  ops() and depth() are the length of the postfix program and the height its stack reaches, as the product compiles
it (FilterCompiler order: operands left to right, then the operator).

columns(n) is the corpus of the two test files: an int column whose dictionary codes are known, a double column and a string column with the values the
coercions of filter.h treat specially."""
import math
import re

import numpy as np

F, T, N = 0, 1, 2


def evaluate(tree, leaf_verdicts):
    """True iff the tree accepts; leaf_verdicts: {leaf text: bool} (`ne` looks up its `field = lit` leaf)."""
    def ev(t):
        k = t[0]
        if k == "leaf":
            return T if leaf_verdicts[t[1]] else F
        if k == "ne":
            return F if leaf_verdicts[eq_leaf(t)] else T
        if k == "lit":
            return N
        if k == "not":
            return F if ev(t[1]) == T else T
        if k == "and":
            l = ev(t[1]); return F if l == F else ev(t[2])
        if k == "or":
            l = ev(t[1]); return T if l == T else ev(t[2])
        c = ev(t[1]); return ev(t[3]) if c == F else ev(t[2])
    return ev(tree) == T


def eq_leaf(t):
    return "%s = %s" % (t[1], t[2])


def leaves(tree, out=None):
    """The leaf texts of a tree, in order of first use."""
    out = [] if out is None else out
    if tree[0] == "leaf":
        out.append(tree[1]) if tree[1] not in out else None
    elif tree[0] == "ne":
        out.append(eq_leaf(tree)) if eq_leaf(tree) not in out else None
    elif tree[0] != "lit":
        for x in tree[1:]:
            leaves(x, out)
    return out


def ops(t):
    return 1 if t[0] in ("leaf", "lit") else 2 if t[0] == "ne" else 1 + sum(ops(x) for x in t[1:])


def depth(t):
    k = t[0]
    if k in ("leaf", "lit", "ne"):
        return 1
    if k == "not":
        return depth(t[1])
    return max(depth(x) + i for i, x in enumerate(t[1:]))


def postfix(t, out=None):
    """The postfix program of a tree as the product compiles it: ("leaf", text), ("lit",), ("not",), ("and",), ("or",), ("tern",)."""
    out = [] if out is None else out
    if t[0] == "leaf":
        out.append(t)
    elif t[0] == "ne":
        out += [("leaf", eq_leaf(t)), ("not",)]
    elif t[0] == "lit":
        out.append(("lit",))
    else:
        for x in t[1:]:
            postfix(x, out)
        out.append((t[0],))
    return out


def device_eval(prog, leaf_verdicts, cap=32):
    """filt_eval_codes (infidex_amd/csrc/filter.hip.inc) restated with its guards: a push beyond `cap` entries is dropped, an operator without its operands
    is skipped.  cap = 32 is the device; a smaller cap is a broken one, which the limit programs must tell apart (tests/test_filter_model.py)."""
    st = []
    for op in prog:
        k = op[0]
        if k in ("leaf", "lit"):
            if len(st) < cap:
                st.append(N if k == "lit" else T if leaf_verdicts[op[1]] else F)
        elif k == "not":
            if st:
                st[-1] = F if st[-1] == T else T
        elif k == "tern":
            if len(st) >= 3:
                b = st.pop(); a = st.pop(); st[-1] = b if st[-1] == F else a
        elif len(st) >= 2:
            r = st.pop(); l = st[-1]
            st[-1] = (F if l == F else r) if k == "and" else (T if l == T else r)
    return bool(st) and st[-1] == T


def kinds(t, out=None):
    """The node kinds of a tree."""
    out = set() if out is None else out
    out.add(t[0])
    if t[0] in ("not", "and", "or", "tern"):
        for x in t[1:]:
            kinds(x, out)
    return out


def text(tree, rng=None, used=None):
    """rng (numpy Generator) mixes the spellings; None prints the keyword forms.  used (a set) collects the spellings chosen: "AND", "&&", "OR", "||",
    "NOT", "!", "!=", "NOT(=)" (a `ne` printed as a negated equality), "?"."""
    pick = (lambda a, b: a if rng.random() < 0.6 else b) if rng is not None else (lambda a, b: a)
    used = set() if used is None else used

    def word(a, b):
        w = pick(a, b); used.add(w); return w

    def p(t, need):
        k = t[0]
        if k in ("leaf", "lit"):
            return t[1]
        if k == "ne":
            if word("!=", "NOT(=)") == "!=":
                s, mine = "%s != %s" % (t[1], t[2]), 4
            else:
                s, mine = "%s (%s)" % (word("NOT", "!"), eq_leaf(t)), 3
        elif k == "not":
            w = word("NOT", "!"); s, mine = (w + " " if w == "NOT" else w) + p(t[1], 3), 3
        elif k == "and":
            s, mine = "%s %s %s" % (p(t[1], 2), word("AND", "&&"), p(t[2], 3)), 2
        elif k == "or":
            s, mine = "%s %s %s" % (p(t[1], 1), word("OR", "||"), p(t[2], 2)), 1
        else:
            used.add("?"); s, mine = "%s ? %s : %s" % (p(t[1], 1), p(t[2], 0), p(t[3], 0)), 0
        return s if mine >= need else "(" + s + ")"
    return p(tree, 0)


LEAF_OPERATORS = ["=", "<", "<=", ">", ">=", "BETWEEN", "IN", "CONTAINS", "STARTS WITH", "ENDS WITH", "LIKE", "IS NULL", "IS NOT NULL"]


def leaf_operator(leaf):
    """The operator token of a leaf text `field <op> constants`."""
    rest = leaf.split(" ", 1)[1]
    for op in ("IS NOT NULL", "IS NULL", "STARTS WITH", "ENDS WITH", "BETWEEN", "CONTAINS", "LIKE", "IN", "<=", ">=", "<", ">", "="):
        if rest == op or rest.startswith(op + " "):
            return op
    raise ValueError(leaf)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------------
def right_nested(kind, xs):
    """x0 OP (x1 OP (x2 ...)): len(xs) operands of depth 1 reach stack depth len(xs)."""
    t = xs[-1]
    for x in reversed(xs[:-1]):
        t = (kind, x, t)
    return t


def left_nested(kind, xs):
    """((x0 OP x1) OP x2) ...: depth 2 whatever the length; n leaves are 2n - 1 ops."""
    t = xs[0]
    for x in xs[1:]:
        t = (kind, t, x)
    return t


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------------------------
INT_VALUES = [5000 + 3 * ((k * 7919) % 1000) for k in range(1000)]      # 1000 distinct values in a scrambled order: value k is first seen at document k
CHOSEN_CODES = [0, 31, 32, 33, 63, 64, 999]                             # around the 32-bit words of a leaf bitmap, and the dictionary's last code
DBL_VALUES = [float("nan"), -0.0, 0.0, 1e15, 1e-5, 1.5, 2.0, 3.0, 7.0, 1000.0, -2.5, 1e14, 0.0001, 123456.789, 250.25, 5.0, -7.0, 0.5, 999999999999999.0, 42.0]
STR_VALUES = ["Drama", "drama", "DRAMA", "", "1,000", " 7 ", "1e3", "7", "1000", "Comedy", "comedy", "Sci-Fi", "sci_fi", "it's", "100%",
              "ǆungla", "Ǆungla", "ǅungla",               # dz-caron digraph: lower, upper, title (Latin Extended-B singles)
              "ὀδός", "Ὀδός",     # Greek Extended
              "ａｂｃ", "ＡＢＣ",                 # fullwidth Latin
              "ⅷ", "Ⅷ",                                         # Roman numeral eight
              "ꙁemlja", "Ꙁemlja",                               # Cyrillic Extended-B
              "აბ", "ᲐᲑ",                             # Georgian Mkhedruli -> Mtavruli
              "ⰰⰱ", "ⰀⰁ"]                             # Glagolitic
# Values whose facet tie order / sort order depends on the case table: a lower-case letter that lies ABOVE the other value while its capital lies BELOW it.
# ASCII a against '_'; Georgian an (10D0 -> Mtavruli 1C90) against Hangul jamo 1100; fullwidth a (FF41 -> FF21) against the fullwidth bracket FF3B.
# Listed ascending by (upper-cased code units, then ordinal) — neither the ordinal order nor the order of str.lower().
FOLD_ORDER = ["ax", "_x", "\u1100b", "\u10d0b", "\uff41x", "\uff3bx"]
INT, DBL, STR, MISSING = "qty", "amt", "tag", "nosuch"


def columns(n=1027):
    """{name: (values, facetable)}: qty int64 (document k < 1000 carries INT_VALUES[k], so its code is k; later documents repeat the chosen codes),
    amt float64, tag str."""
    qty = np.asarray([INT_VALUES[k] if k < 1000 else INT_VALUES[CHOSEN_CODES[k % len(CHOSEN_CODES)]] for k in range(n)], np.int64)
    amt = np.asarray([DBL_VALUES[(5 * k + k // len(DBL_VALUES)) % len(DBL_VALUES)] for k in range(n)], np.float64)
    tag = [STR_VALUES[(7 * k + k // len(STR_VALUES)) % len(STR_VALUES)] for k in range(n)]
    return {INT: (qty, True), DBL: (amt, False), STR: (tag, True)}


def quote(s, rng=None):
    """A literal token for the string s: bare when the lexer reads it as a number (digits and '.'), else quoted."""
    if re.fullmatch(r"[0-9][0-9.]*", s) and (rng is None or rng.random() < 0.7):
        return s
    return '"%s"' % s if "'" in s else "'%s'" % s


def number_text(v):
    """How a column value reads as a literal: repr without a trailing '.0'."""
    if isinstance(v, float):
        if math.isnan(v):
            return "NaN"
        s = repr(float(v))
        return s[:-2] if s.endswith(".0") else s
    return str(v)


def code_leaves():
    """One `qty = v` leaf per chosen code: the bit of that code, alone in its bitmap."""
    return [("leaf", "%s = %d" % (INT, INT_VALUES[c])) for c in CHOSEN_CODES]


def leaf_pool(rng, per_kind=6):
    """Leaves over columns() covering every operator of the grammar, an unknown field, and constants that meet the coercions."""
    q = lambda s: quote(s, rng)
    ints = sorted(INT_VALUES)
    out = [t[1] for t in code_leaves()]
    for _ in range(per_kind):
        a, b = sorted(int(x) for x in rng.choice(ints, 2, replace=False))
        out += ["%s %s %d" % (INT, op, a) for op in rng.choice(["<", "<=", ">", ">="], 2, replace=False)]
        out.append("%s BETWEEN %d AND %s" % (INT, a, q(str(b))))
        out.append("%s IN (%s)" % (INT, ", ".join(str(int(x)) for x in rng.choice(ints, int(rng.integers(1, 40)), replace=False))))
        out.append("%s LIKE '%s%%'" % (INT, str(a)[:2]))
        out.append("%s ENDS WITH %s" % (INT, q(str(a)[-1])))
        d = [number_text(x) for x in rng.choice(DBL_VALUES, 3, replace=False)]
        out += ["%s %s %s" % (DBL, op, q(d[0])) for op in rng.choice(["=", "<", "<=", ">", ">="], 2, replace=False)]
        out.append("%s BETWEEN %s AND %s" % (DBL, q(d[1]), q(d[2])))
        out.append("%s IN (%s)" % (DBL, ", ".join(q(x) for x in d)))
        s = [str(x) for x in rng.choice([v for v in STR_VALUES if v], 3, replace=False)]
        flip = s[0].swapcase() if rng.random() < 0.5 else s[0]
        out.append("%s = %s" % (STR, q(flip)))
        out += ["%s %s %s" % (STR, op, q(s[1])) for op in rng.choice(["<", "<=", ">", ">="], 2, replace=False)]
        out.append("%s IN (%s)" % (STR, ", ".join(q(x.upper() if rng.random() < 0.5 else x) for x in s)))
        out.append("%s CONTAINS %s" % (STR, q(s[2][1:3].upper())))
        out.append("%s STARTS WITH %s" % (STR, q(s[1][:2].swapcase())))
        out.append("%s ENDS WITH %s" % (STR, q(s[0][-2:].lower())))
        out.append("%s LIKE %s" % (STR, q(rng.choice(["%" + s[2][1:].upper(), s[1][:1] + "%", "_" + s[0][1:].lower(), "%" + s[2][1:2] + "%", "_____", "%"]))))
        out.append("%s BETWEEN %s AND %s" % (STR, q(min(s[0], s[1])), q(max(s[0], s[1]))))
    out += ["%s IS NULL" % STR, "%s IS NOT NULL" % STR, "%s IS NULL" % DBL, "%s IS NOT NULL" % INT, "%s IS NULL" % MISSING, "%s IS NOT NULL" % MISSING,
            "%s = 1" % MISSING, "%s < 5" % MISSING, "%s >= 5" % MISSING, "%s CONTAINS 'a'" % MISSING,
            "%s = '1000'" % STR, "%s < 8" % STR, "%s >= '1E3'" % STR, "%s = '1E+15'" % DBL, "%s = '1E-05'" % DBL, "%s = '-0'" % DBL, "%s = 0" % DBL,
            "%s <= 'NaN'" % DBL, "%s > 'nan'" % DBL, "%s = 'dRAMA'" % STR, "%s LIKE 'Ǆ%%'" % STR, "%s STARTS WITH 'Ὀ'" % STR,
            "%s = 'ＡＢＣ'" % STR, "%s CONTAINS 'Ⅷ'" % STR, "%s = 'ᲐᲑ'" % STR, "%s ENDS WITH 'EMLJA'" % STR]
    seen = []
    for x in out:
        if x not in seen:
            seen.append(x)
    return seen


NE_OPERANDS = [(INT, str(INT_VALUES[31])), (INT, str(INT_VALUES[64])), (DBL, "'NaN'"), (DBL, "0"), (DBL, "1.5"), (STR, "'DRAMA'"), (STR, "'7'"), (STR, "''"),
               (STR, "'ǄUNGLA'"), (MISSING, "3")]
LITERALS = ["1", "0", "'true'", "'x'", "2.5", '"no"']


def random_tree(rng, pool, size):
    """A tree of about `size` operands drawn from pool (leaf texts), with `ne`, literals, NOT, AND, OR and ternaries mixed in."""
    if size <= 1:
        r = rng.random()
        if r < 0.08:
            return ("lit", str(rng.choice(LITERALS)))
        if r < 0.2:
            f, v = NE_OPERANDS[int(rng.integers(len(NE_OPERANDS)))]
            return ("ne", f, v)
        return ("leaf", str(pool[int(rng.integers(len(pool)))]))
    r = rng.random()
    if r < 0.12:
        return ("not", random_tree(rng, pool, size))
    if r < 0.27 and size >= 3:
        a = int(rng.integers(1, size - 1)); b = int(rng.integers(1, size - a))
        return ("tern", random_tree(rng, pool, a), random_tree(rng, pool, b), random_tree(rng, pool, size - a - b))
    a = int(rng.integers(1, size))
    return ("and" if rng.random() < 0.45 else "or", random_tree(rng, pool, a), random_tree(rng, pool, size - a))


def qty_eq(code):
    return ("leaf", "%s = %d" % (INT, INT_VALUES[code]))


def qty_ne(code):
    return ("ne", INT, str(INT_VALUES[code]))


def or_chain(d, start, step):
    """qty = v0 OR (qty = v1 OR (...)) over d distinct codes: stack depth d, accepts exactly the documents that carry one of the codes — every operand
    position decides a document, so an operand lost or garbled anywhere in the stack drops one."""
    return right_nested("or", [qty_eq((start + i * step) % 1000) for i in range(d)])


def and_chain(d, start, step):
    """qty != v0 AND (qty != v1 AND (...)), every operand a bool: depth d, rejects exactly the documents that carry one of the d codes."""
    return right_nested("and", [qty_ne((start + i * step) % 1000) for i in range(d)])


LIMIT_SHAPES = [(63, 32), (95, 32), (255, 2), (256, 2), None, (17, 9), (47, 16), (33, 17), (93, 31)]      # (ops, depth) of limit_trees, None: depth 32 only


def limit_trees(rng, pool):
    """The programs at the limits — stack depth exactly 32 (an OR chain, an AND chain and ternaries nested in the else branch), 255 and 256 ops at depth 2 —
    and chains at the depths between what random trees reach and the limit (9, 16, 17, 31).  Every leaf of the chains picks one dictionary code of its own
    (the OR chain's codes 0, 31, 62 ... are spread over the words of the leaf bitmap), so each program accepts some documents and rejects others, and a
    program cut short at any op, or a stack that loses any entry, changes the accepted set."""
    leaf = lambda: ("leaf", str(pool[int(rng.integers(len(pool)))]))
    out = [or_chain(32, 0, 31), and_chain(32, 7, 29),
           left_nested("or", [qty_eq((3 + 7 * i) % 1000) for i in range(128)]),                        # 255 ops, depth 2
           ("and", left_nested("or", [qty_eq((5 + 7 * i) % 1000) for i in range(127)]), qty_ne(5 + 7 * 60))]      # 253 + 2 + 1 = 256 ops, depth 2
    t = qty_eq(999)                                                                                 # c ? a : (c ? a : (...)): the else branch sits two slots up
    for i in range(15):
        t = ("tern", qty_eq(40 + i), leaf(), t)
    out.append(("or", qty_eq(64), t))                                                               # 1 + (2 * 15 + 1) = 32
    out += [or_chain(9, 2, 111), and_chain(16, 11, 61), or_chain(17, 1, 57), ("not", and_chain(31, 4, 32))]
    assert len(out) == len(LIMIT_SHAPES)
    for x, want in zip(out, LIMIT_SHAPES):
        assert (ops(x), depth(x)) == want if want else depth(x) == 32, (ops(x), depth(x), want)
    return out


def over_limit_trees(pool):
    """Programs the device must refuse: stack depth 33, and 257 ops."""
    leaf = lambda i: ("leaf", str(pool[i % len(pool)]))
    deep = right_nested("and", [leaf(i) for i in range(33)])
    long_ = left_nested("or", [leaf(i) for i in range(129)])
    assert depth(deep) == 33 and ops(deep) == 65 and ops(long_) == 257 and depth(long_) == 2
    return deep, long_


N_FIXED = len(LIMIT_SHAPES) + len(CHOSEN_CODES)      # the programs every generate() starts with


def generate(seed, count, pool=None, used=None):
    """count trees: the limit programs, one single-leaf tree per chosen code, then random ones of 2..24 operands.  Returns (trees, texts); used collects the
    spellings text() chose."""
    rng = np.random.default_rng(seed)
    pool = leaf_pool(rng) if pool is None else pool
    trees = limit_trees(rng, pool) + code_leaves()
    while len(trees) < count:
        trees.append(random_tree(rng, pool, int(rng.integers(2, 25))))
    trees = trees[:count]
    return trees, [text(t, rng, used) for t in trees]
