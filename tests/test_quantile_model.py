"""The selection of field_quantiles (infidex_amd/csrc/quantile_select.h on listing_select.h and set_walk.h) without a GPU: the three headers, UNCHANGED,
compiled with g++ into tests/models/quantile_model.cpp, which walks the whole multi-target select serially the way k_quant_hist and k_quant_pick do —
histogram, pick, histogram, ... for every (slot, quantile) at once, the pick by 64 parts of a row as the wave takes them, or by one — and compares every
target with a plain sort of its slot's keys.

Walked there: every digit width from 4 to 11; nvals at 2^k - 2, 2^k - 1, 2^k and 2^k + 1 (the select's bits are those of nvals + 1, so the number of
passes changes between the first two); keys up to 31 bits; one member, all keys equal, two keys that part only at the last digit; q of 0 and 1, sixteen
unsorted q with duplicates; groups without a member; a mask that accepts nothing and one that accepts the last document only; NaN ranks.  The program runs
under the address and undefined-behaviour sanitizers (host code with its own main) on heap blocks of exactly n elements.

qs_position — the one floating-point operation of the feature — is held to Python's math.floor((c - 1) * q)."""
import math
import os
import random
import struct
import subprocess

import pytest

from infidex_amd import QuantileRequest      # (the feature these headers belong to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quantile") / "quantile_model")
    # -Wno-unknown-pragmas: set_walk.h's `#pragma unroll` is the kernels'
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "models", "quantile_model.cpp"), "-o", exe])
    return exe


def test_every_target_equals_a_plain_sort(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    # selects, targets compared, slots whose targets part at the last digit only, slots without a non-NaN member, slots of one member
    assert f[0] == "OK" and int(f[1]) > 3000 and int(f[2]) > 100000 and int(f[3]) > 0 and int(f[4]) > 0 and int(f[5]) > 0, out.stdout
    assert QuantileRequest().q == (0.5,)


def test_the_position_is_pythons_floor_of_one_double_product(model):
    qs = [0.0, 2.0 ** -1074, 0.1, 1 / 3, 0.5, 1 - 2.0 ** -53, 1.0]
    rng = random.Random(5)
    counts = sorted({1, 2, 3, 4, 7, 10, 11, 100, 1000, 4099, 2 ** 31 - 2, 2 ** 31 - 1} | {2 ** k + d for k in range(2, 31) for d in (-1, 0, 1)}
                    | {rng.randrange(1, 2 ** 31) for _ in range(3000)})
    pairs = [(c, q) for c in counts for q in qs] + [(rng.randrange(1, 2 ** 31), rng.random()) for _ in range(20000)]
    text = "".join("%d %d\n" % (c, struct.unpack("<Q", struct.pack("<d", q))[0]) for c, q in pairs)
    out = subprocess.run([model, "pos"], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [int(x) for x in out.stdout.split()]
    assert len(got) == len(pairs)
    want = [math.floor((c - 1) * q) for c, q in pairs]
    assert got == want, [(p, g, w) for p, g, w in zip(pairs, got, want) if g != w][:5]
    assert max(want) == 2 ** 31 - 2 and min(want) == 0


def test_headers_have_no_hip_types_and_reuse_the_listing_arithmetic():
    """The kernels include the very files the model compiles; the digit arithmetic is listing_select.h's, not a copy of it."""
    src = open(os.path.join(CSRC, "quantile_select.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic"):
        assert word not in src, word
    assert '#include "listing_select.h"' in src
    for name in ("ls_passes", "ls_shift", "ls_digit", "ls_under_prefix", "ls_extend", "ls_pick"):
        assert "uint32_t %s(" % name not in src and "bool %s(" % name not in src, name
    kernels = open(os.path.join(CSRC, "quantiles.hip.inc")).read()
    assert '#include "quantile_select.h"' in kernels and '#include "set_walk.h"' in kernels
    for name in ("ls_shift", "ls_digit", "ls_under_prefix", "qs_step", "qs_start", "qs_key", "sw_flags16", "sw_codes16", "sw_member"):
        assert name + "(" in kernels, name
    assert '#include "quantiles.hip.inc"' in open(os.path.join(CSRC, "infidex_hip.hip")).read()
