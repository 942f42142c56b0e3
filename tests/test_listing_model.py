"""The arithmetic of list_documents' selection (infidex_amd/csrc/listing_select.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/listing_model.cpp, which walks the whole select serially the way the kernels do — a histogram of the current digit under each target's
prefix, the pick of the digit that holds the target's position, ..., the thresholds and tie indices, the three key classes, each wanted document's slot,
a sort of the page — and compares every page element for element with a plain sort of (key, document).

Walked there: digit widths 4, 5 and 11; key ranges of 1 to 32 bits (keys up to 2^32 - 2: three 11-bit and eight 4-bit passes, which no GPU test of a few
seconds reaches); both directions; offsets 0, at the first element of the longest tie, inside it, at its last element, at total - 1, at total and beyond,
and 2^31 - 1; limits 1, 97 and 1024; an empty set; all keys equal; all keys distinct; two heavy keys that differ in one chosen digit only, for every digit —
the program itself fails unless the first and last position of some page parted at every pass of every pass count, and never."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("listing") / "listing_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "models", "listing_model.cpp"), "-o", exe])
    return exe


def test_select_equals_a_plain_sort(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    assert f[0] == "OK" and int(f[1]) == int(f[2]) and int(f[1]) > 40000, out.stdout


def test_header_has_no_hip_types():
    """The kernels include the very file the model compiles: nothing in it may need the HIP headers."""
    src = open(os.path.join(CSRC, "listing_select.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__"):
        assert word not in src, word
    assert '#include "listing_select.h"' in open(os.path.join(CSRC, "listing.hip.inc")).read()
