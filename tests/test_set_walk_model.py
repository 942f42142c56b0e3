"""The set walk (infidex_amd/csrc/set_walk.h) without a GPU: the header, UNCHANGED, compiled with g++ into tests/models/set_walk_model.cpp, which reads the
16 documents of a thread the way k_list_hist, k_range_counts, k_field_stats and k_group_heads do — sw_flags16, sw_any4, sw_member, sw_codes16 — and compares
every flag byte, every membership and every code with a definition written byte by byte.

Walked there: every corpus of 1 to 48 documents, every group of 16 that begins inside it and the first one beyond; a null mask, all 2^16 flag patterns of the
group that holds the last document, 4096 random ones of every other; a null column.  Flags and codes are heap blocks of exactly n elements and the program runs
under the address and undefined-behaviour sanitizers (host code with its own main): a read at or beyond n fails it."""
import os
import subprocess

import pytest

from infidex_amd import ListRequest, RangeRequest, StatsRequest, GroupListRequest      # (the features this header belongs to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")
WALKERS = ("listing.hip.inc", "ranges.hip.inc", "stats.hip.inc", "groups.hip.inc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("set_walk") / "set_walk_model")
    # -Wno-unknown-pragmas: the header's `#pragma unroll` is the kernels'
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "models", "set_walk_model.cpp"), "-o", exe])
    return exe


def test_flags_members_and_codes_equal_their_definition_and_nothing_is_read_beyond_the_corpus(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    # per n the groups that begin inside the corpus and one beyond: 16 x (2 + 3 + 4); per group the null mask, then 2^16 patterns of each n's last group,
    # 4096 of the 16 x (0 + 1 + 2) other groups, 16 of each n's group beyond
    patterns = 144 + 48 * 65536 + 48 * 4096 + 48 * 16
    assert f[0] == "OK" and int(f[1]) == 144 and int(f[2]) == patterns and int(f[3]) == 16 * patterns, out.stdout
    assert ListRequest().limit == GroupListRequest().limit == 20 and RangeRequest().edges == () and StatsRequest().group_by is None


def test_header_has_no_hip_types_and_every_walk_includes_it():
    """The kernels include the very file the model compiles: nothing in it may need the HIP headers.  And it is the only reader: the four files that walk
    include it and carry no reader of their own."""
    src = open(os.path.join(CSRC, "set_walk.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic"):
        assert word not in src, word
    hip = open(os.path.join(CSRC, "infidex_hip.hip")).read()
    for name in WALKERS:
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "set_walk.h"' in text and '#include "%s"' % name in hip, name
        for gone in ("rng_mask16", "grp_mask16", "grp_member", "sts_codes16", "0x01010101u) & ~"):
            assert gone not in text, (name, gone)
