"""The arithmetic of range_facets' counting pass (infidex_amd/csrc/range_buckets.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/range_model.cpp, which looks up every rank 0 .. nvals the way k_range_counts does — rb_slot over the request's thresholds — and compares it
with a linear scan of the thresholds.

Walked there: 1, 2, 3, 7, 8, 100, 255 and 256 buckets; thresholds with runs of equal values (empty buckets), all equal at the bottom, in the middle and at
the top; thr[0] = 0 (nothing below) and thr[B] = nvals (nothing above); nanRanks 0 and 1; nvals of 1, 2, 3, 100 and 2^17.  The program itself fails
unless the slots partition the ranks as the thresholds say and the widest lookup reads nine thresholds."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ranges") / "range_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "models", "range_model.cpp"), "-o", exe])
    return exe


def test_lookup_equals_a_linear_scan(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    # 5 sizes x 8 bucket counts x 2 nanRanks (less the impossible ones) x 11 threshold sets; 2^17 + 1 ranks for each of the large ones
    assert f[0] == "OK" and int(f[1]) > 800 and int(f[2]) > 100 * (1 << 17), out.stdout


def test_header_has_no_hip_types():
    """The kernel includes the very file the model compiles: nothing in it may need the HIP headers."""
    src = open(os.path.join(CSRC, "range_buckets.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic"):
        assert word not in src, word
    assert '#include "range_buckets.h"' in open(os.path.join(CSRC, "ranges.hip.inc")).read()
    assert '#include "ranges.hip.inc"' in open(os.path.join(CSRC, "infidex_hip.hip")).read()
