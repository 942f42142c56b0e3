"""The span walk and the window choice of Query.highlight (infidex_amd/csrc/highlight.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/highlight_model.cpp, which holds hl_span_walk to a recount and hl_window to a brute force over every (start word, end word) pair.

Walked there: 0, 1, 2, 63, 64, 65, 191 and 192 words; 0, 1, 63, 64 and 65 matched words (65: truncation); widths 16, 160 and 512; all spans of one term and
spans of distinct terms; words that end in a surrogate pair; a word longer than the width (matched or not; first, in the middle, last; alone).  The stand-alone
program runs plain and under the address and undefined-behaviour sanitizers; nothing is loaded into Python.  The Python model's window (tests/highlight_model.py)
is held to the same rule on its own cases here."""
import os
import random
import subprocess

from infidex_amd import Query
from tests import highlight_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")
WANT = ["OK", str(8 * 5 * 2 * 3 * 3 + 3 * 3 * 2 + 3)]      # counts x marks x term layouts x repeats x widths + the long words


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp("highlight") / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(HERE, "models", "highlight_model.cpp"), "-o", exe])
    return exe


def run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.split() == WANT, out.stdout


def test_the_walk_and_the_window_equal_a_brute_force(tmp_path_factory):
    assert Query("x", highlight=True).highlight_chars == 160      # (the feature this header belongs to)
    run(build(tmp_path_factory, "model", ["-O2"]))


def test_they_stay_in_their_arrays_under_the_address_sanitizer(tmp_path_factory):
    assert Query("x", highlight=True, highlight_chars=16).highlight_chars == 16
    run(build(tmp_path_factory, "model_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_header_has_no_hip_types_and_the_kernel_includes_it():
    assert Query("x").highlight is False
    src = open(os.path.join(CSRC, "highlight.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "__syncthreads", "atomic"):
        assert word not in src, word
    inc = open(os.path.join(CSRC, "highlight.hip.inc")).read()
    assert '#include "highlight.h"' in inc
    for fn in ("hl_span_walk(", "hl_window(", "hl_row_u16("):
        assert fn in inc and fn in src, fn
    hip = open(os.path.join(CSRC, "infidex_hip.hip")).read()
    assert hip.index('#include "stage2.hip.inc"') < hip.index('#include "highlight.hip.inc"')      # (the tokeniser and the comparisons are stage2.hip.inc's)


def test_the_python_window_follows_the_rule():
    # "aa bb cc dd ee": words at 0, 3, 6, 9, 12.  One span at "cc" (6), width 16: the window [6, 14) holds cc dd ee (8 units), 8 unused, budget 2: no
    # word starts within 2 units before 6 (bb starts at 3), so it stays.
    raw = [(0, 2), (3, 2), (6, 2), (9, 2), (12, 2)]
    assert M.window(raw, [(6, 2, 6, 2, 0)], 16) == (6, 8)
    # width 32: 24 unused, budget 6: the earliest word start within 6 units is 0
    assert M.window(raw, [(6, 2, 6, 2, 0)], 32) == (0, 14)
    # two terms beat two spans of one term; equal ranks: the earliest
    spans = [(0, 2, 0, 2, 0), (3, 2, 3, 2, 0), (9, 2, 9, 2, 1), (12, 2, 12, 2, 0)]
    assert M.window(raw, spans, 5) == (9, 5)
    assert M.window(raw, [], 5) == (0, 5) and M.window([], [], 16) == (0, 0)
    assert M.window([(2, 40)], [(2, 40, 2, 40, 0)], 16) == (2, 16)      # a word longer than the width: its first 16 units
    rng = random.Random(7)
    for _ in range(200):          # against the definition, spelled out once more
        raw = []; at = 0
        for _ in range(rng.randint(1, 30)):
            at += rng.randint(1, 3); ln = rng.randint(2, 12); raw.append((at, ln)); at += ln
        spans = [(o, l, o, l, rng.randrange(4)) for o, l in raw if rng.random() < 0.3]
        width = rng.choice([16, 40, 160])
        best = None
        for a in [s[0] for s in spans] or [raw[0][0]]:
            e = a + width
            fit = [o + l for o, l in raw if o >= a and o + l <= a + width]
            if fit:
                e = fit[-1]
            rank = (len({s[4] for s in spans if a <= s[0] < e}), sum(1 for s in spans if a <= s[0] < e))
            if best is None or rank > best[0]:
                best = (rank, a, e)
        _, a, e = best
        b = next((o for o, _ in raw if o < a and a - o <= (width - (e - a)) // 4), a)
        assert M.window(raw, spans, width) == (b, e - b)
