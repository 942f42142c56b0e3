"""k_stage2's fusion arithmetic held to the oracle's bits.

1. A hand-written corpus whose candidates reach every branch of FusionScorer.Calculate / ComputeSemanticScore (oracle/coverage.hpp fusion_calculate), every
   k_stage2 launch (fast <= 32 words, retry 33-192, the pool pass beyond 192, the long-query launches beyond 32 distinct query words) and quirk Q18 (a query of
   more than 255 characters contained in one of the first two documents: the partner row's recomputed SumCi), on the plain and on the ALIAS instantiation.
   The branch guard decodes what the oracle's trace reached (orc_trace_branches) and fails when the corpus stops covering a branch.  The lower semantic clamp
   (`semantic < 0`) is not in the list: every term of the semantic score (per-term coverage, density, bonuses, the non-negative BM25 share) is >= 0.
2. The Stage-2 launch variants (INFX_S2_POOL, INFX_S2_WAVES) agree bit for bit, one fresh process per variant.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle_lib as O

WORDS26 = ["stargazer", "moonlight", "sunflower", "waterfall", "rainforest", "thunderbolt", "snowflake", "butterfly", "dragonfly", "honeycomb", "lighthouse",
           "marshmallow", "nightingale", "pineapple", "quicksilver", "rattlesnake", "saltwater", "tumbleweed", "underwater", "wildflower", "yellowtail",
           "blackberry", "cornflower", "driftwood", "evergreen", "firefly"]
Q18_QUERY = " ".join(WORDS26)                       # 26 distinct words, > 255 characters: the fast envelope, LCS above a byte
BASE_DOCS = [
    "apple", "green apple pie", "applesauce recipe book", "fresh applesauce", "red apple tree", "red apple",
    "zebra crossing the street", "the street of the city", "running shoes for men", "runner shoes sale",
    "spider man swings through new york", "spider monkey in the zoo", "a b", "of to in",
    "quantum physics lecture notes", "quantum mechanics and the physics of light", "lecture hall schedule",
    "dark knight rises", "the dark knight returns", "knight in shining armour",
    "ocean blue waves", "blue ocean strategy book", "deep ocean blue whale",
    "xylophone music lessons", "music lessons for kids", "the music of the night",
    "new york city guide", "new jersey turnpike", "york minster cathedral",
    "the " + Q18_QUERY + " story",                                                        # Q18: contains the 26-word query
    "music lessons " + " ".join(f"tone{i}" for i in range(60)),                           # 62 words: the retry launch
    "ocean blue " + " ".join(f"wave{i % 150} tide{i}" for i in range(130)),               # 262 words: the pool pass
    "blue whale " + " ".join(f"tone{i}" for i in range(0, 120, 3)),                       # 42 words
]
QUERIES = ["apple", "appl", "red apple", "red apple tree", "red apple tree house", "zebra street", "zebra the", "running shoes", "runn shoes",
           "spider m", "spider man", "quantum physics lecture", "quantum physics lec", "dark knight", "dark knight ri", "the dark knight zzz",
           "ocean blue", "blue ocean whale", "xylophone lessons", "music lessons kids zzz", "new york", "new york city guide book map",
           "a b c", "of to in zz", "quantum zzz yyy xxx", "quantum physics zzz yyy", "apple pie green fresh", "deep ocean blue whale",
           "knight armour", "knight in sh", "music of the ni", "quant phys lect", "quantum physics lecture notes hall", "new y",
           "apple appl", "knight knigh", "york yor", "red apple app", "ocean wave7 tide12", "music tone3 tone40",
           Q18_QUERY, " ".join(f"tone{i}" for i in range(40)), " ".join(f"tone{i}" for i in range(0, 120, 3)) + " whale"]
ALIAS_DOC = "ſtraße lang µm filter"         # OrdinalIgnoreCase alias characters (long s, micro sign): the corpus runs k_stage2's ALIAS instantiation
REQUIRED = [b for b in O.FUSION_BRANCHES if b != "clamp_low"] + ["doc<=32", "doc33-192", "doc>192", "query>32", "q18"]


def corpus(alias):
    docs = list(BASE_DOCS) + ([ALIAS_DOC] if alias else [])
    return list(enumerate(docs))


def reached(o, docs, queries):
    """Branches and launches the oracle's trace shows for `queries` (the corpus must be indexed in `o`)."""
    words = {k: len(t.split()) for k, t in docs}
    seen = set()
    o.set_trace(True)
    for q in queries:
        o.search(q, 10)
        ids, base, sc, ties, feat = o.last_trace()
        for i in range(len(ids)):
            seen |= o.trace_branches(i)
            n = words[int(ids[i])]
            seen.add("doc<=32" if n <= 32 else ("doc33-192" if n <= 192 else "doc>192"))
            if len(set(q.split())) > 32:
                seen.add("query>32")
            if feat[i, 24] > 255 and list(ids).count(ids[i]) == 2:
                seen.add("q18")                     # LCS above a byte on a document evaluated twice (WordMatcher overlap row, then its Stage-1 row)
    o.set_trace(False)
    return seen


@pytest.mark.parametrize("alias", [False, True], ids=["plain", "alias"])
def test_fusion_corpus_reaches_every_branch(alias):
    docs = corpus(alias)
    o = O.OracleEngine.create_default(); o.index(docs)
    seen = reached(o, docs, QUERIES)
    assert not [b for b in REQUIRED if b not in seen], [b for b in REQUIRED if b not in seen]


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [False, True], ids=["plain", "alias"])
def test_fusion_branches_bit_exact_on_gpu(alias):
    from infidex_amd import Document
    from tests.test_gpu_parity import compare_batch, gpu_engine
    docs = corpus(alias)
    o = O.OracleEngine.create_default(); o.index(docs)
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    st = compare_batch(e, o, QUERIES, 10)
    print("fusion corpus", "alias" if alias else "plain", st)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0 and st["s1_boundary"] == 0, st
    assert st["s2_rows"] > 500, st
    seen = reached(o, docs, QUERIES)
    assert not [b for b in REQUIRED if b not in seen], [b for b in REQUIRED if b not in seen]
    print("branches reached:", sorted(seen))


VARIANT_SCRIPT = r'''
import sys, numpy as np
from infidex_amd import SearchEngine
from infidex_amd.engine import pack_texts
from tools.synth import Synth
s = Synth(2, docs=40000); arena, offs = s.docs()
texts = Synth.texts(arena, offs)
longs = [" ".join(texts[i:i + n]) for i, n in zip(range(0, 2000, 50), [6, 12, 20, 40, 80, 160] * 7)]          # 40 documents of ~50 to ~1300 words
texts = texts + longs
e = SearchEngine.create_default(device=0, want_features=True)
a, o = pack_texts(texts); e.index_flat(None, a, o)
e.delete_documents(np.arange(0, len(texts), 11))
qa, qo = s.queries(300, qseed=71, fuzz=0.5)
qs = Synth.texts(qa, qo)
qs += [" ".join(dict.fromkeys(w for t in qs[:30] for w in t.split())), longs[3][:300].rsplit(" ", 1)[0], longs[9], " ".join(longs[5].split()[:12])]
qa, qo = pack_texts(qs)
k, sc, t, c, f = e.search_packed(qa, qo, 10)
q2, d2, b2, s2, t2, f2 = e.last_stage2()
np.savez(sys.argv[1], k=k, sc=sc.view(np.uint32), t=t, c=c, f=f, q2=q2, d2=d2, b2=b2.view(np.uint32), s2=s2.view(np.uint32), t2=t2, f2=f2)
'''


@pytest.mark.gpu
def test_stage2_launch_variants_agree_bit_for_bit(tmp_path):
    """The fast launch's LDS text pool (INFX_S2_POOL: 0 = texts in global memory, 64 = most lanes do not fit and read global memory, 32768) and its register
    budget (INFX_S2_WAVES = 2 / 4 / 8 waves per SIMD; default 6) change where k_stage2 reads and how it is scheduled, never what it computes: final rows and
    every Stage-2 row (base, score, tie, all 32 feature ints) are identical, on a fuzzy batch with deletions, long documents and long queries."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variants = [dict(), dict(INFX_S2_POOL="0"), dict(INFX_S2_POOL="64"), dict(INFX_S2_POOL="32768"),
                dict(INFX_S2_WAVES="2"), dict(INFX_S2_WAVES="4"), dict(INFX_S2_WAVES="8")]
    res = []
    for vi, var in enumerate(variants):
        env = dict(os.environ); env.update(var)
        env["PYTHONPATH"] = root
        out = str(tmp_path / f"s2_{vi}.npz")
        subprocess.run([sys.executable, "-c", VARIANT_SCRIPT, out], check=True, env=env, timeout=600, cwd=root)
        res.append(np.load(out))
    assert res[0]["q2"].size > 5000 and int(res[0]["c"].sum()) > 2000
    for var, other in zip(variants[1:], res[1:]):
        for key in res[0].files:
            assert np.array_equal(res[0][key], other[key]), (var, key)
