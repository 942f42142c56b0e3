"""The wide entry point of the device introsort (bcl_introsort_wide in infidex_amd/csrc/bclsort.hip.inc, run by k_postproc_wide over up to 1024 rows)
as host code: the SAME source file compiled with g++ and checked element for element against oracle/dotnet.hpp's IntroSorter at
n in {65, 127, 128, 129, 255, 256, 257, 511, 512, 1000, 1023, 1024} on tie-heavy inputs with the three comparisons of k_postproc, and on a McIlroy
adversary input at n = 1024 that reaches the heapsort fallback.  The model's dump also holds the Python port (tests/bcl_sort.py), with which the GPU
tests compute their expected rows, to the same order at these sizes.  The device code is checked on the GPU by tests/test_gpu_post_rows.py."""
import os
import struct
import subprocess

import pytest

from tests import bcl_sort as B

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (65, 127, 128, 129, 255, 256, 257, 511, 512, 1000, 1023, 1024)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bclsort_wide") / "bclsort_wide_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(HERE, "models", "bclsort_wide_model.cpp"), "-o", exe])
    return exe


def test_wide_device_sort_equals_the_bcl_restatement(model):
    out = subprocess.run([model, "40"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-2000:] + out.stderr[-2000:]
    sorts, insertion, partition, heapsort, deepest = (int(x) for x in out.stdout.split()[1:6])
    assert sorts == len(SIZES) * 3 * 40 + 2
    assert insertion > 0 and partition > 0 and heapsort > 0, out.stdout       # heapsort: only the adversary input at n = 1024 gets there
    assert 1 <= deepest <= 23                                                  # 2 * (log2 1024 + 1) + 1 pending ranges at the most


def test_python_port_equals_the_wide_device_sort(model):
    out = subprocess.run([model, "dump", "13", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    seen = set()
    for line in out.stdout.splitlines():
        head, tail = line.split("|")
        f = head.split()
        mode, n = int(f[0]), int(f[1])
        vals = f[2:2 + n]
        want = [int(x) for x in tail.split()]
        if mode == 0:
            sc = [struct.unpack("<f", bytes.fromhex(v)[::-1])[0] for v in vals]
            got = B.introsort(list(range(n)), lambda a, b: B.cmp_float(sc[b], sc[a]))
        else:
            key = [None if int(v) == 0 else int(v) for v in vals]
            if mode == 1:
                got = B.introsort(list(range(n)), lambda a, b: B.cmp_values(key[a], key[b]))
            else:
                got = B.introsort(list(range(n)), lambda a, b: B.cmp_values(key[b], key[a]))
        assert got == want, (mode, n)
        seen.add((mode, n))
    assert seen == {(m, n) for m in range(3) for n in SIZES}
