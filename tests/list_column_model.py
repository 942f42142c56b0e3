"""A plain Python model of list columns (SearchEngine.set_list_column) for the GPU tests: the constructed corpus, any-element filter leaves and facet counts.

An expression is a tree: ("leaf", column, op, args) over a list column, ("scalar", column, op, value) over an int scalar column, ("not", x), ("and", x, y),
("or", x, y).  text() spells it in the filter language, holds() walks it for one document.  The leaf operators are the ones whose coercions are trivial
on the corpus below — ints compared as numbers, lower-case ASCII strings compared as they are; the coercion corners are tests/test_list_columns_model.py's.
An empty list is a null value: IS NULL holds, `<` holds (FilterVM orders a null below every constant, as for a scalar field), nothing else does."""
from collections import Counter

from tests.browse_model import order_facets

N = 1031                                   # not a multiple of 4, 64 or 256
VOCAB = ["t%02d" % i for i in range(32)]   # with "" the dictionary of `tags` holds 33 values
EMPTY_RUN = range(100, 170)                # 70 consecutive empty lists
DUPLICATES = 7                             # the document whose elements are all one value
DELETED = [5, 64, 257, 900]


def tags_lists():
    out = []
    for d in range(N):
        if d in (0, N - 1) or d in EMPTY_RUN:
            out.append([])
        elif d == 1:
            out.append(["t01"])
        elif d in (2, 3, 4):
            out.append([VOCAB[j % 31] for j in range({2: 63, 3: 64, 4: 65}[d])])
        elif d == 6:
            out.append([VOCAB[(j * 5) % 31] for j in range(300)])      # longer than a workgroup's share of elements
        elif d == DUPLICATES:
            out.append(["t05"] * 5)
        elif d == 8:
            out.append(["", "t02"])
        elif d == 9:
            out.append([""])
        else:
            out.append([VOCAB[(d * 3 + j * 7) % 32] for j in range(d % 5)])
    return out


def int_lists(values, per_doc):
    """Lists over the ints 0 .. values - 1: document d holds per_doc(d) elements, taken in turn."""
    out, i = [], 0
    for d in range(N):
        k = 0 if d in (0, N - 1) else per_doc(d)
        out.append([(i + j) % values for j in range(k)])
        i += k
    return out


def corpus(big_values):
    """{name: (lists, facetable)}: dictionaries of 33 (strings), 1, 31, 32 and big_values (one above the kernel's LDS bitmap budget) values, and a column
    whose every list is empty."""
    return {
        "tags": (tags_lists(), True),
        "one": ([[0] * (d % 4) for d in range(N)], False),
        "v31": (int_lists(31, lambda d: d % 3), False),
        "v32": (int_lists(32, lambda d: (d * 7) % 5), True),
        "big": (int_lists(big_values, lambda d: 64), True),
        "none": ([[] for _ in range(N)], True),
    }


def year_of(d):
    return 2000 + d % 7


def text(x):
    if x[0] == "leaf":
        _, col, op, args = x
        q = lambda v: "'%s'" % v if isinstance(v, str) else str(v)
        if op == "BETWEEN":
            return "%s BETWEEN %s AND %s" % (col, q(args[0]), q(args[1]))
        if op == "IN":
            return "%s IN (%s)" % (col, ", ".join(q(v) for v in args))
        if op == "IS NULL":
            return "%s IS NULL" % col
        return "%s %s %s" % (col, op, q(args[0]))
    if x[0] == "scalar":
        return "%s %s %d" % (x[1], x[2], x[3])
    if x[0] == "not":
        return "NOT (%s)" % text(x[1])
    return "(%s) %s (%s)" % (text(x[1]), x[0].upper(), text(x[2]))


def leaf_holds(op, args, elements):
    if op == "!=":                                        # the parser lowers it to NOT over an = leaf: no element equals (an empty list has none)
        return not leaf_holds("=", args, elements)
    if not elements:                                      # a null value
        return op in ("IS NULL", "<")
    if op == "=":
        return any(e == args[0] for e in elements)
    if op == "<":
        return any(e < args[0] for e in elements)
    if op == ">=":
        return any(e >= args[0] for e in elements)
    if op == "BETWEEN":
        return any(args[0] <= e <= args[1] for e in elements)
    if op == "IN":
        return any(e in args for e in elements)
    if op == "CONTAINS":
        return any(args[0] in e for e in elements)
    if op == "STARTS WITH":
        return any(e.startswith(args[0]) for e in elements)
    if op == "IS NULL":
        return any(e == "" for e in elements)
    raise ValueError(op)


def holds(x, columns, d):
    if x[0] == "leaf":
        return leaf_holds(x[2], x[3], columns[x[1]][0][d])
    if x[0] == "scalar":
        v = year_of(d)
        return {"=": v == x[3], "<": v < x[3], ">=": v >= x[3]}[x[2]]
    if x[0] == "not":
        return not holds(x[1], columns, d)
    a, b = holds(x[1], columns, d), holds(x[2], columns, d)
    return (a and b) if x[0] == "and" else (a or b)


def accepted(x, columns, deleted=()):
    """The live documents the expression accepts, ascending."""
    dead = set(deleted)
    return [d for d in range(N) if d not in dead and holds(x, columns, d)]


def facets(columns, docs):
    """{field: [(value, count)]} of the facetable list columns over `docs`: element occurrences, empty strings left out, ordered and cut as the scalar facets."""
    out = {}
    for name, (lists, facetable) in columns.items():
        if not facetable:
            continue
        c = Counter(str(e) for d in docs for e in lists[d] if e != "")
        if c:
            out[name] = order_facets(dict(c))
    return out
