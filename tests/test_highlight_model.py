"""tests/highlight_model.py — the Python restatement of Query.highlight that the GPU tests hold k_highlight to — pinned to the oracle, without a GPU.

The oracle does not say which document word a query word matched, but oracle_lib.coverage_standalone(query, doc) returns eleven features that the model's
records determine (highlight_model.FEATURES).  They are derived from the records (highlight_model.features, the code the GPU cross-check against k_stage2 uses
too) and must equal the oracle's on constructed pairs that reach each of the six recording sites and every branch inside them, and on 400 seeded random
pairs, among which every kind occurs at least ten times."""
import random

import pytest

from tests import highlight_model as M
from tests import oracle_lib

# (query, stored text, the kinds of the query's words in order)
CASES = [
    ("alpha", "alpha beta", ["whole"]),
    ("beta alpha", "alpha beta", ["whole", "whole"]),
    ("new york", "newyork city", ["joined_query", "joined_query"]),
    ("big new york", "a newyork city", ["none", "joined_query", "joined_query"]),
    ("newyork", "new york", ["joined_doc"]),
    ("newyork city", "the city of new york", ["joined_doc", "whole"]),
    ("alph", "alphabet", ["prefix"]),
    ("bet", "alphabet", ["suffix"]),
    ("phab", "alphabet", ["infix"]),
    ("pha", "alphabet", ["none"]),                       # an infix needs four characters
    ("alphabet", "bet", ["tail"]),
    ("alpx", "alphabet", ["fuzzy_prefix"]),              # the prefix of the query word's length, distance 1
    ("alph", "xlphabet", ["fuzzy_prefix"]),
    ("alhab", "alphabet", ["fuzzy_prefix"]),             # one longer
    ("alxpha", "alphabet", ["fuzzy_prefix"]),            # one shorter
    ("al", "xyphabet", ["none"]),                        # a last word of two characters is offered, this one does not match
    ("ax", "alphabet", ["fuzzy_prefix"]),                # ... this one does, at distance 1
    ("ax beta", "alphabet beta", ["none", "whole"]),     # ... and is not offered when it is not the last word
    ("alphabex", "alphabet", ["fuzzy"]),                 # distance 1
    ("alhpa", "alpha", ["fuzzy"]),                       # a transposition counts 1
    ("alphxbex", "alphabet", ["fuzzy"]),                 # distance 2, from seven characters on
    ("alxhxb", "alphab", ["none"]),                      # six characters: one typo only
    ("ab", "ax", ["fuzzy"]),                             # the two-letter special case: same first letter
    ("ab", "xb", ["none"]),
    ("alpha alph", "alpha", ["whole", "none"]),          # the whole-word matcher took the word: the prefix matcher is not offered it
    ("alph alpha", "alpha", ["none", "whole"]),
    ("alpha", "", ["none"]),
    ("alpha beta gamma", "gamma x beta alphabet", ["prefix", "whole", "whole"]),
]
EXPECT = {"alpx": (4, 1), "alhab": (6, 1), "alxpha": (5, 1)}      # fuzzy_prefix: (match_length, distance)


def check(query, doc):
    h = M.highlight(query, doc)
    assert h["status"] == "ok"
    _, feat, _, _ = oracle_lib.coverage_standalone(query, doc)
    got = M.features(h["terms"], h["words"])
    want = {k: feat[k] for k in M.FEATURES}
    assert got == want, (query, doc, h["terms"])
    assert feat["TermsCount"] == len(h["terms"])
    return h


@pytest.mark.parametrize("query,doc,kinds", CASES)
def test_constructed_pairs_reach_every_site_and_agree_with_the_oracle(query, doc, kinds):
    h = check(query, doc)
    assert [t["kind"] for t in h["terms"]] == kinds
    if query in EXPECT:
        assert (h["terms"][0]["match_length"], h["terms"][0]["distance"]) == EXPECT[query]
    for t in h["terms"]:
        if t["kind"] != "none":
            d = M.units(doc)
            assert M.text_of(d[t["offset"]:t["offset"] + t["length"]]) in doc.split()
            assert t["offset"] <= t["match_offset"] and t["match_offset"] + t["match_length"] <= t["offset"] + t["length"]
    if kinds == ["fuzzy"]:
        assert h["terms"][0]["distance"] == (2 if query == "alphxbex" else 1)


def test_records_of_the_sub_ranges():
    t = M.highlight("phab", "an alphabet")["terms"][0]
    assert (t["offset"], t["length"], t["match_offset"], t["match_length"]) == (3, 8, 5, 4)
    t = M.highlight("bet", "an alphabet")["terms"][0]
    assert (t["match_offset"], t["match_length"]) == (8, 3)
    a, b = M.highlight("new york", "in newyork")["terms"]
    assert (a["offset"], a["match_offset"], a["match_length"]) == (3, 3, 3) and (b["offset"], b["match_offset"], b["match_length"]) == (3, 6, 4)
    t = M.highlight("newyork", "new  york")["terms"][0]
    assert (t["offset"], t["length"], t["offset2"], t["length2"], t["match_length"]) == (0, 3, 5, 4, 3)


def random_pair(rng):
    alphabet = "abcde"
    word = lambda lo, hi: "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))
    docw = [word(2, 9) for _ in range(rng.randint(1, 6))]
    qw = []
    for _ in range(rng.randint(1, 3)):
        w = rng.choice(docw); op = rng.randrange(12)
        if op == 0:
            qw.append(w)
        elif op == 1:
            qw.append(w[:rng.randint(2, max(2, len(w) - 1))])
        elif op == 2:
            qw.append(w[-rng.randint(2, max(2, len(w) - 1)):])
        elif op == 3 and len(w) >= 6:
            qw.append(w[1:5])
        elif op == 4:
            qw.append(word(1, 3) + w)
        elif op in (5, 6, 7):                                       # one or two edits, or an edited prefix
            x = list(w if op != 7 else w[:max(4, len(w) - 2)])
            for _ in range(1 if op != 6 else 2):
                x[rng.randrange(len(x))] = rng.choice(alphabet)
            qw.append("".join(x))
        elif op == 8 and len(docw) >= 2:
            k = rng.randrange(len(docw) - 1); qw.append(docw[k] + docw[k + 1])
        elif op == 9 and len(w) >= 4:
            k = rng.randint(2, len(w) - 2); qw += [w[:k], w[k:]]
        elif op == 10:
            x = list(w); k = rng.randrange(len(x)); del x[k]; qw.append("".join(x) if len(x) >= 2 else w)
        else:
            qw.append(word(2, 8))
    return " ".join(qw), rng.choice([" ", "  ", ", ", "-"]).join(docw)


def test_random_pairs_agree_with_the_oracle_and_use_every_kind():
    rng = random.Random(20260317)
    seen = {k: 0 for k in M.KINDS}
    for _ in range(400):
        q, d = random_pair(rng)
        for t in check(q, d)["terms"]:
            seen[t["kind"]] += 1
    assert all(n >= 10 for n in seen.values()), seen
