"""The oracle with a settable CoverageSetup — TEST INFRASTRUCTURE ONLY.

oracle/coverage.hpp and oracle/pipeline.hpp honour every member of CoverageSetup, but the oracle's C ABI has no setter.  tests/models/oracle_coverage_setup.cpp
includes oracle/oracle_c.cpp and adds one; this module builds it with the Makefile's flags into a temporary directory (as tests/test_lev_model.py builds its
model) and hands out OracleEngines bound to it (oracle_engine()); tests.oracle_lib itself keeps its own library.

Engine-wide setup: set_setup(o, cs).  Per-query setup: search(o, text, ..., query_setup=cs) writes the six members SearchPipeline reads (pipeline.hpp:131-204;
coverage.hpp reads none of them) around that one search and restores them — the matcher members of a query's setup are ignored, as in the reference.

Also here: the inputs and the setups of the coverage-setup tests (tests/test_coverage_setup_api.py, tests/test_gpu_coverage_setup*.py).
"""
import ctypes as C
import dataclasses
import hashlib
import os
import re
import subprocess
import tempfile

import numpy as np

from infidex_amd import CoverageSetup
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = os.path.join(ROOT, "tests", "models", "oracle_coverage_setup.cpp")
PIPELINE_FIELDS = ("truncate", "coverage_min_word_hits_abs", "coverage_min_word_hits_relative", "truncation_score",
                   "coverage_q_limit_for_error_tolerance", "coverage_lcs_error_tolerance_relativeq")

_shim = None


def _makefile_flags():
    txt = open(os.path.join(O.ORACLE_DIR, "Makefile")).read()
    return re.search(r"^CXXFLAGS \?= (.*)$", txt, re.M).group(1).split()


def build_shim():
    """Compiles the shim once per state of its sources (about 25 s); later calls, other test modules and other processes of the run find it built."""
    srcs = [SHIM_SRC] + sorted(os.path.join(O.ORACLE_DIR, f) for f in os.listdir(O.ORACLE_DIR) if f.endswith((".hpp", ".cpp")))
    h = hashlib.sha256()
    for s in srcs:
        h.update(open(s, "rb").read())
    d = os.path.join(tempfile.gettempdir(), "infidex_oracle_shim_%d_%s" % (os.getuid(), h.hexdigest()[:16]))
    os.makedirs(d, mode=0o700, exist_ok=True)
    lib = os.path.join(d, "liboracle_setup.so")
    if not os.path.exists(lib):
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        subprocess.check_call([os.environ.get("CXX", "g++"), *_makefile_flags(), "-shared", "-o", tmp, SHIM_SRC, "-lpthread"])
        os.replace(tmp, lib)           # complete or absent, whoever else builds it at the same time
    return lib


def use_shim():
    """Loads the shim (a superset of liboracle.so) with the restype / argtypes set-up of tests.oracle_lib; the module's own library stays what it was."""
    global _shim
    if _shim is None:
        path = build_shim()
        keep = (O.LIB_PATH, O._lib)
        try:
            O.LIB_PATH, O._lib = path, None
            _shim = O.lib()
        finally:
            O.LIB_PATH, O._lib = keep
        _shim.orc_set_coverage_setup.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_double]
        _shim.orc_set_coverage_setup.restype = None
    return _shim


def oracle_engine(**kw):
    """An OracleEngine bound to the shim (engines made elsewhere keep tests.oracle_lib's library)."""
    shim = use_shim()
    keep = O._lib
    try:
        O._lib = shim                  # OracleEngine.__init__ takes its library from oracle_lib.lib()
        o = O.OracleEngine(**kw) if kw else O.OracleEngine.create_default()
    finally:
        O._lib = keep
    assert o.L is shim
    o._setup = CoverageSetup()
    return o


def set_setup(o, cs: CoverageSetup):
    """The oracle's engine-wide CoverageSetup."""
    v = np.asarray([cs.min_word_size, cs.levenshtein_max_word_size, cs.num_typos, cs.min_length_one_typo, cs.min_length_two_typos,
                    cs.coverage_min_word_hits_abs, cs.coverage_min_word_hits_relative, cs.coverage_q_limit_for_error_tolerance,
                    int(cs.cover_whole_query), int(cs.cover_whole_words), int(cs.cover_fuzzy_words), int(cs.cover_joined_words), int(cs.cover_prefix_suffix),
                    int(cs.truncate), cs.truncation_score], np.int32)
    use_shim().orc_set_coverage_setup(o.h, v.ctypes.data_as(C.POINTER(C.c_int32)), float(cs.coverage_lcs_error_tolerance_relativeq))
    o._setup = cs


def pipeline_override(engine_setup: CoverageSetup, query_setup: CoverageSetup) -> CoverageSetup:
    """What a query with its own setup runs under: the engine's matchers, the query's six pipeline-level members."""
    return dataclasses.replace(engine_setup, **{f: getattr(query_setup, f) for f in PIPELINE_FIELDS})


def search(o, text, k=10, depth=500, query_setup=None, **kw):
    """OracleEngine.search under the engine-wide setup, or — query_setup — with that query's pipeline-level members written for this search only."""
    if query_setup is None:
        return o.search(text, k, depth, **kw)
    base = o._setup
    set_setup(o, pipeline_override(base, query_setup))
    try:
        return o.search(text, k, depth, **kw)
    finally:
        set_setup(o, base)


def answer(r):
    """Keys, score bits and tiebreakers of a result."""
    return (tuple(r["keys"]), tuple(np.asarray(r["scores"], np.float32).view(np.uint32).tolist()), tuple(int(t) for t in r["ties"]))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def synth_corpus():
    from tools.synth import Synth
    s = Synth(2, docs=40000)
    arena, offs = s.docs()
    return s, arena, offs


def set_s1(s):
    from tools.synth import Synth
    return Synth.texts(*s.queries(120, qseed=43, fuzz=0.3))


def set_s2(s):
    """300 queries, the first word of each of the first 100, and each of the first 100 cut by two characters but never below four: 500 texts."""
    from tools.synth import Synth
    q = Synth.texts(*s.queries(300, qseed=5, fuzz=0.5))
    return q + [t.split()[0] for t in q[:100]] + [t[:max(4, len(t) - 2)] for t in q[:100]]


HAND_TITLES = ["new york city guide", "newyork pizza", "new york", "york new", "batman begins", "bat man returns", "batman", "the dark knight rises",
               "dark knight", "shaw shank", "shawshank redemption", "super man", "superman returns", "inter stellar travel", "interstellar",
               "spider man homecoming", "spiderman", "iron man", "ironman three", "star wars", "starwars saga", "lord of the rings", "thelord rings",
               "new yorker magazine"]
HAND_FILLER = ["%s %s number %d" % (a, b, i) for i, (a, b) in enumerate(
    [(a, b) for a in ("quiet", "river", "stone", "garden", "winter", "copper", "lantern", "harbor") for b in ("story", "atlas", "letters", "manual", "diary")])]
HAND_DOCS = list(enumerate(HAND_TITLES + HAND_FILLER))          # 24 titles + 40 filler lines = 64 documents
HAND_QUERIES = ["newyork", "new york", "batman", "bat man", "superman", "super man", "inter stellar", "interstellar", "shawshank", "shaw shank",
                "spiderman", "spider man", "ironman", "iron man", "starwars", "star wars", "darkknight rises", "thelord of rings"]
assert len(HAND_DOCS) == 64 and len(HAND_QUERIES) == 18

# CoverageMinWordHitsAbs decides here: one query word of three matches, the two first Stage-1 documents neither start like the query nor contain it (LCS 0)
# and score below TruncationScore (no tier bit), so the last surviving row qualifies by its word hits alone
MINHITS_DOCS = list(enumerate(["xx%d lantern item%d" % (i, i) for i in range(12)] + ["unrelated text %d" % i for i in range(20)]))
MINHITS_QUERIES = ["lantern qqqqq zzzzz", "lantern qqqqq zzzzz wwwww"]

# ---- the setups under test: (name, setup) per input set ----------------------------------------------------------------------------------------------
D = CoverageSetup
SETUPS_S1 = [
    ("minimal", D.create_minimal()),
    ("fuzzy-off", D(cover_fuzzy_words=False)),
    ("typos-0", D(num_typos=0)),
    ("typo-lengths-5-10", D(min_length_one_typo=5, min_length_two_typos=10)),
    ("prefix-suffix-off", D(cover_prefix_suffix=False)),
    ("whole-words-off", D(cover_whole_words=False)),
    ("min-word-size-3", D(min_word_size=3)),
    ("lev-max-word-6", D(levenshtein_max_word_size=6)),
    ("truncate-off", D(truncate=False)),
]
SETUPS_S2 = [
    ("two-typos-from-5", D(min_length_two_typos=5)),
    ("typos-1", D(num_typos=1)),
    ("whole-query-off", D(cover_whole_query=False)),
    ("relativeq-0.9", D(coverage_lcs_error_tolerance_relativeq=0.9)),
    ("relativeq-0.0", D(coverage_lcs_error_tolerance_relativeq=0.0)),
    ("qlimit-50", D(coverage_q_limit_for_error_tolerance=50)),
    ("truncation-score-0", D(truncation_score=0)),
]
SETUPS_HAND = [
    ("joined-off", D(cover_joined_words=False)),
    ("truncate-off", D(truncate=False)),
]
# On S1, S2 and the hand corpus none of these alone changes an answer: there they are held to "equal to the oracle".  MINHITS_DOCS / MINHITS_QUERIES is an
# input on which CoverageMinWordHitsAbs 2 and 3 do; no input was found on which CoverageMinWordHitsRelative alone does.
SETUPS_MIN_HITS = [("min-hits-abs-%d" % a, D(coverage_min_word_hits_abs=a)) for a in (2, 3, 4)] + [("min-hits-rel-%d" % r, D(coverage_min_word_hits_relative=r)) for r in (1, 3)]
