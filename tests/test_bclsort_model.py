"""The introsort k_postproc runs for Query.Boosts / Query.SortBy (infidex_amd/csrc/bclsort.hip.inc) as host code: the SAME source file compiled with g++
and checked element for element against oracle/dotnet.hpp's IntroSorter (ArraySortHelper<T>.IntrospectiveSort) for every n in 0..64 on tie-heavy
inputs with the three comparisons of k_postproc, and on an input that reaches the heapsort fallback.  The model's output also pins the Python port
(tests/bcl_sort.py) the GPU tests compute their expected rows with.  The device code is checked on the GPU by tests/test_gpu_boost_sort.py."""
import os
import struct
import subprocess

import pytest

from tests import bcl_sort as B

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bclsort") / "bclsort_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(HERE, "models", "bclsort_model.cpp"), "-o", exe])
    return exe


def test_device_sort_equals_the_bcl_restatement(model):
    out = subprocess.run([model, "300"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-2000:] + out.stderr[-2000:]
    sorts, insertion, partition, heapsort = (int(x) for x in out.stdout.split()[1:5])
    assert sorts == 65 * 3 * 300 + 2
    assert insertion > 0 and partition > 0 and heapsort > 0, out.stdout


def test_python_port_equals_the_device_sort(model):
    out = subprocess.run([model, "dump", "11", "3000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    big = 0
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
        assert got == want, line
        big += n > 16
    assert big > 1000


def test_python_port_apply_steps():
    """apply_boosts: fp32 add only where the total boost is positive, then the score-descending sort even when nothing was boosted (rows with equal
    scores move); apply_sort: nulls first ascending and last descending, and descending is not the reverse of ascending."""
    rows = [(k, 0.5, 0) for k in range(20)]
    plain = B.apply_boosts(list(rows), [[] for _ in rows])
    assert sorted(plain) == rows and plain != rows                       # 20 equal scores: the unstable introsort permutes them
    boosted = B.apply_boosts(list(rows), [[3] if k == 7 else [] for k in range(20)])
    assert boosted[0] == (7, 3.5, 0)
    x = float(2 ** 24 + 1)
    assert B.apply_boosts([(1, 2.0 ** 24, 0)], [[1]])[0][1] == 2.0 ** 24 != x     # rounds as an fp32 add
    keys = [None, 3, 1, None, 2] * 4
    asc = B.apply_sort(list(range(20)), keys, True)
    desc = B.apply_sort(list(range(20)), keys, False)
    assert [keys[i] for i in asc][:8] == [None] * 8 and [keys[i] for i in desc][-8:] == [None] * 8
    assert desc != asc[::-1]
    assert B.string_key("Drama") != B.string_key("drama") and B.string_key("Drama") < B.string_key("drama") < B.string_key("Fantasy")
    assert B.double_key(-0.0) == B.double_key(0.0) and B.double_key(float("nan")) < B.double_key(-1e308)
