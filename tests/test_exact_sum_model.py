"""The arithmetic of field_stats' exact sums (infidex_amd/csrc/exact_sum.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/exact_sum_model.cpp, which does what the kernel and the engine do with it — the column's scale, every value's limbs added into signed 64-bit
sums, the sums recombined, rounded once, divided by the count — and prints every figure.  Here each figure is held to fractions.Fraction (the exact real
sum and quotient; float(Fraction) rounds once to nearest-even, subnormals included) and, where the values can be written out, to math.fsum.

Cases: random doubles whose spread needs 1, 2, 3 and 4 limbs; subnormals; +-0.0; total cancellation; a spread of exactly 128 binary digits (summable) and
of 129 (refused); sums beyond the double range (+-inf); +-inf and NaN members; ties at the rounding bit of the sum and of the mean; 2^31 - 1 occurrences
of the largest limb (no limb sum overflows); int64 with INT64_MIN / INT64_MAX repeated until the sum needs more than 64 bits."""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")
INT, DBL = 1, 2
INF = float("inf")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exact_sum") / "exact_sum_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "models", "exact_sum_model.cpp"), "-o", exe])
    return exe


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def dbl_of(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def run(model, cases):
    """cases: [(kind, [(value, times)])], value a float or an int -> the model's output lines, split"""
    text = []
    for kind, vals in cases:
        text.append("%d %d" % (kind, len(vals)))
        text += ["%016x %d" % (bits_of(v) if kind == DBL else v & (2 ** 64 - 1), t) for v, t in vals]
    out = subprocess.run([model], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = [l.split() for l in out.stdout.splitlines()]
    assert len(lines) == len(cases)
    return lines


def rounded(fr):
    """fr rounded once to nearest-even, beyond the double range +-inf"""
    try:
        return float(fr)
    except OverflowError:
        return INF if fr > 0 else -INF


def span(vals):
    """(scale, bits) of the finite non-zero values: lowest and highest exponent of a set bit"""
    lo = hi = None
    for v, _ in vals:
        if isinstance(v, float) and (math.isnan(v) or math.isinf(v)):
            continue
        fr = abs(Fraction(v))
        if not fr:
            continue
        l = -(fr.denominator.bit_length() - 1) if fr.denominator > 1 else (fr.numerator & -fr.numerator).bit_length() - 1
        h = fr.numerator.bit_length() - fr.denominator.bit_length()
        h = h if Fraction(2) ** h <= fr else h - 1
        lo = l if lo is None else min(lo, l); hi = h if hi is None else max(hi, h)
    return (0, 1) if lo is None else (lo, 1 + hi - lo)


def check(kind, vals, f):
    """one output line f of the model against the exact arithmetic"""
    scale, bits = span(vals)
    if kind == INT:
        scale = 0; bits = max([abs(v).bit_length() for v, _ in vals] + [1])
    L = (bits + 31) // 32
    summable = L <= (2 if kind == INT else 4)
    assert int(f[0]) == int(summable) and int(f[1]) == scale and int(f[2]) == L, (f, scale, bits)
    if not summable:
        return
    fin = [(v, t) for v, t in vals if kind == INT or not (math.isnan(v) or math.isinf(v))]
    nan = sum(t for v, t in vals if kind == DBL and math.isnan(v))
    pinf = sum(t for v, t in vals if kind == DBL and v == INF); ninf = sum(t for v, t in vals if kind == DBL and v == -INF)
    exact = sum((Fraction(v) * t for v, t in fin), Fraction(0))
    S = [int(x) for x in f[3:7]]
    assert all(-2 ** 63 <= s < 2 ** 63 for s in S) and all(s == 0 for s in S[L:])
    assert Fraction(2) ** scale * sum(s << (32 * i) for i, s in enumerate(S)) == exact                 # the limb sums ARE the sum
    count = sum(t for _, t in fin) + pinf + ninf
    assert (int(f[7]), int(f[8]), int(f[9]), int(f[10])) == (count, nan, pinf, ninf)
    got_sum = dbl_of(int(f[11], 16))
    if pinf or ninf:
        want = float("nan") if pinf and ninf else (INF if pinf else -INF)
        assert math.isnan(got_sum) if math.isnan(want) else got_sum == want
        if count:
            got_mean = dbl_of(int(f[12], 16))
            assert math.isnan(got_mean) if math.isnan(want) else got_mean == want
        return
    assert got_sum == rounded(exact) and (exact != 0 or int(f[11], 16) == 0), (got_sum, rounded(exact))     # a zero sum is +0.0
    if count:
        assert dbl_of(int(f[12], 16)) == rounded(exact / count), (dbl_of(int(f[12], 16)), rounded(exact / count))
    else:
        assert f[12] == "-"
    if kind == INT:
        got = (int(f[13], 16) << 64 | int(f[14], 16))
        assert (got - (1 << 128) if got >> 127 else got) == exact
    if kind == DBL and sum(t for _, t in fin) <= 4096 and abs(exact) < Fraction(2) ** 1023:
        assert got_sum == math.fsum(v for v, t in fin for _ in range(t))


def random_doubles(rng, limbs, n):
    """n doubles whose set bits lie within a window of 32 * limbs binary digits, both signs"""
    base = rng.randrange(-1000, 900 - 32 * limbs)
    out = []
    for _ in range(n):
        width = rng.randrange(1, 54)
        e = rng.randrange(base, base + 32 * limbs - width + 1) if 32 * limbs > width else base
        m = rng.getrandbits(width) | 1 | (1 << (width - 1))
        if width > 32 * limbs:
            m &= (1 << (32 * limbs)) - 1; m |= 1
        out.append((math.ldexp(float(m), e) * rng.choice((1, -1)), rng.randrange(1, 4)))
    return out


def test_random_doubles_of_one_to_four_limbs(model):
    rng = random.Random(20261019)
    cases = []
    for limbs in (1, 2, 3, 4):
        for n in (1, 2, 17, 300):
            for _ in range(6):
                cases.append((DBL, random_doubles(rng, limbs, n)))
    for (kind, vals), f in zip(cases, run(model, cases)):
        check(kind, vals, f)
    assert {int(f[2]) for f in run(model, cases)} == {1, 2, 3, 4}


def test_edges_of_the_double_format(model):
    tiny = 5e-324                                        # 2^-1074
    cases = [
        (DBL, [(tiny, 1)]), (DBL, [(tiny, 3), (-tiny, 1)]), (DBL, [(tiny * 3, 5), (2.0 ** -1022, 1), (2.0 ** -1030 * 5, 7)]),      # subnormals
        (DBL, [(0.0, 3), (-0.0, 2)]), (DBL, [(-0.0, 1)]), (DBL, []),                                                             # zeroes, nothing
        (DBL, [(1.5, 2), (-3.0, 1)]), (DBL, [(1e9, 60), (-1e9, 60), (2.0 ** -20, 1), (-(2.0 ** -20), 1)]),                       # total cancellation
        (DBL, [(2.0 ** 127, 1), (1.0, 1)]), (DBL, [(2.0 ** 128, 1), (1.0, 1)]),                                                  # 128 digits; 129: refused
        (DBL, [(2.0 ** -1074, 1), (2.0 ** -947, 1)]), (DBL, [(2.0 ** -1074, 1), (2.0 ** -946, 1)]),
        (DBL, [(1e-30, 1), (1e30, 1)]),                                                                                          # refused
        (DBL, [(2.0 ** 1023, 2)]), (DBL, [(-(2.0 ** 1023), 3), (2.0 ** 1000, 1)]), (DBL, [(1.7976931348623157e308, 1), (2.0 ** 971, 1)]),      # beyond the range
        (DBL, [(1.7976931348623157e308, 1), (2.0 ** 970, 1)]),                                                                   # a tie at the very top: to even = inf
        (DBL, [(1.7976931348623157e308, 1), (2.0 ** 969, 1)]),                                                                   # just below it: stays finite
        (DBL, [(2.0 ** 1023, 2), (-(2.0 ** 1023), 1)]),                                                                          # the sum fits, the partial sum would not
        (DBL, [(INF, 1), (1.0, 2)]), (DBL, [(-INF, 2), (1.0, 2)]), (DBL, [(INF, 1), (-INF, 1), (2.0, 1)]), (DBL, [(float("nan"), 4)]),
        (DBL, [(float("nan"), 4), (2.5, 2), (INF, 1)]),
    ]
    lines = run(model, cases)
    for (kind, vals), f in zip(cases, lines):
        check(kind, vals, f)
    assert [int(f[0]) for f in lines[8:13]] == [1, 0, 1, 0, 0]
    assert dbl_of(int(lines[13][11], 16)) == INF and dbl_of(int(lines[14][11], 16)) == -INF and dbl_of(int(lines[15][11], 16)) == INF and dbl_of(int(lines[16][11], 16)) == INF
    assert dbl_of(int(lines[17][11], 16)) == 1.7976931348623157e308 and dbl_of(int(lines[18][11], 16)) == 2.0 ** 1023


def test_ties_at_the_rounding_bit(model):
    cases = [
        (DBL, [(2.0 ** 53, 1), (1.0, 1)]),               # 2^53 + 1: a tie, to even (down)
        (DBL, [(2.0 ** 53, 1), (3.0, 1)]),               # 2^53 + 3: a tie, to even (up)
        (DBL, [(2.0 ** 53, 1), (1.0, 1), (2.0 ** -40, 1)]),      # just above the tie: up
        (DBL, [(2.0 ** 53, 1), (3.0, 1), (-(2.0 ** -40), 1)]),   # just below the tie: down
        (DBL, [(-(2.0 ** 53), 1), (-1.0, 1)]), (DBL, [(-(2.0 ** 53), 1), (-3.0, 1)]),
        (DBL, [(2.0 ** 54, 1), (2.0, 1)]),               # mean of two: (2^54 + 2) / 2 = 2^53 + 1, a tie
        (DBL, [(2.0 ** 54, 1), (6.0, 1)]),               # 2^53 + 3
        (DBL, [(2.0 ** 54, 1), (1.0, 2)]),               # mean of three: not a dyadic fraction, sticky
        (DBL, [(1.0, 1), (2.0, 1), (4.0, 1)]), (DBL, [(1.0, 7)]), (DBL, [(0.1, 3)]), (DBL, [(5e-324, 1), (0.0, 1)]), (DBL, [(5e-324, 3), (0.0, 1)]),
        (DBL, [(5e-324, 1), (0.0, 2)]),                  # a third of the smallest subnormal: to zero
        (INT, [(2 ** 53, 1), (1, 1)]), (INT, [(2 ** 53 + 1, 1), (2 ** 53 + 2, 1)]), (INT, [(1, 1), (0, 2)]), (INT, [(-1, 1), (0, 2)]),
    ]
    for (kind, vals), f in zip(cases, run(model, cases)):
        check(kind, vals, f)


def test_limb_sums_do_not_overflow_and_int64_extremes(model):
    top = 2 ** 31 - 1
    cases = [
        (DBL, [(float(2 ** 32 - 1), top)]),                              # the largest limb, 2^31 - 1 times
        (DBL, [(-float(2 ** 32 - 1), top)]),
        (DBL, [(float(2 ** 32 - 1) * 2.0 ** 96 + 0.0, top - 1), (1.0, 1)]),      # in the fourth limb
        (DBL, [(float(2 ** 53 - 1) * 2.0 ** 75, top - 1), (1.0, 1)]),
        (INT, [(2 ** 63 - 1, top)]), (INT, [(-2 ** 63, top)]),           # beyond 64 bits
        (INT, [(2 ** 63 - 1, 3), (-2 ** 63, 1)]), (INT, [(2 ** 63 - 1, 1000), (-2 ** 63, 1000)]), (INT, [(-2 ** 63, 1)]), (INT, [(2 ** 63 - 1, 2)]),
        (INT, [(0, 5)]), (INT, []), (INT, [(7, 3), (-9, 2), (2 ** 40, 1)]), (INT, [(2 ** 32, 1)]), (INT, [(2 ** 32 - 1, 1)]),
    ]
    lines = run(model, cases)
    for (kind, vals), f in zip(cases, lines):
        check(kind, vals, f)
    assert int(lines[4][13], 16) != 0 and int(lines[5][13], 16) != 2 ** 64 - 1      # the int128's upper half is in use
    assert [int(f[2]) for f in lines[10:15]] == [1, 1, 2, 2, 1]


def test_header_has_no_hip_types():
    """The kernel includes the very file the model compiles: nothing in it may need the HIP headers."""
    src = open(os.path.join(CSRC, "exact_sum.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic"):
        assert word not in src, word
    assert '#include "exact_sum.h"' in open(os.path.join(CSRC, "stats.hip.inc")).read()
    assert '#include "stats.hip.inc"' in open(os.path.join(CSRC, "infidex_hip.hip")).read()
    assert '#include "../exact_sum.h"' in open(os.path.join(CSRC, "host", "engine.cpp")).read()
