"""The arithmetic of list_groups' passes (infidex_amd/csrc/group_heads.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/group_model.cpp, which looks group codes up among a page's sorted codes the way k_group_sizes does — gh_find — and compares every lookup with a
linear scan, and holds the composite (key << 32 | document) to the order of (key, document) pairs.

Walked there: code lists of 0, 1, 2, 3, 7, 8, 9, 511, 512, 513, 1023 and 1024 entries — dense from code 0, dense up to the largest code, with gaps, random —
each asked for every code it holds, both neighbours of each, codes at and beyond both ends and random ones.  The program itself fails unless the widest lookup
reads eleven codes."""
import os
import subprocess

import pytest

from infidex_amd import GroupListRequest      # (the feature this header belongs to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("groups") / "group_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "models", "group_model.cpp"), "-o", exe])
    return exe


def test_lookup_equals_a_linear_scan_and_composites_order_as_pairs(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    # 12 sizes x 11 lists; per list 3 lookups per code + 70; 200 000 composite pairs
    assert f[0] == "OK" and int(f[1]) == 12 * 11 and int(f[2]) > 12 * 11 * 70 + 3 * 11 * 1024 and int(f[3]) == 200000, out.stdout
    assert GroupListRequest().limit == 20


def test_header_has_no_hip_types():
    """The kernels include the very file the model compiles: nothing in it may need the HIP headers."""
    src = open(os.path.join(CSRC, "group_heads.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic"):
        assert word not in src, word
    assert '#include "group_heads.h"' in open(os.path.join(CSRC, "groups.hip.inc")).read()
    assert '#include "groups.hip.inc"' in open(os.path.join(CSRC, "infidex_hip.hip")).read()
