"""The arithmetic of field_distinct (infidex_amd/csrc/distinct_set.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/distinct_model.cpp, which holds it to std::set and plain loops:

  * pair index, row stride, word and bit address: every pair of G x V has a bit of its own inside its row (V at and around multiples of 32), on a heap block of
    exactly the bitmap's size; the 2^32-bit limit;
  * the capacity rule: a power of two, at least 2 x the pairs, no larger than needed, at least the minimum size;
  * the probe sequence: `capacity` distinct slots, consecutive modulo the capacity — keys that start at the table's last slots wrap around;
  * ds_insert against std::set: new exactly once per key, however often it comes; the GPU tests' two shapes (4 099 members into 7 and into 4 099 pairs);
    a full chain of 512 colliding keys, also across the table's end;
  * the bounded loop: on a deliberately undersized, full table every further key visits each slot once and reports DS_OVERFLOW, and the table is unchanged.
    (Host only: the device's table is sized never to fill, and no GPU test tries to make it.)

The program runs under the address and undefined-behaviour sanitizers (host code with its own main)."""
import os
import subprocess

import pytest

from infidex_amd import DistinctRequest      # (the feature this header belongs to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("distinct") / "distinct_model")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "models", "distinct_model.cpp"), "-o", exe])
    return exe


def test_addresses_capacities_probes_and_inserts_equal_plain_code(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    # pair addresses, capacities, probe steps, inserts held to std::set, the longest chain walked, overflows reported
    assert f[0] == "OK" and int(f[1]) > 500000 and int(f[2]) > 40 and int(f[3]) > 500000 and int(f[4]) > 100000 and int(f[5]) == 512 and int(f[6]) == 200, out.stdout
    assert DistinctRequest().field is None


def test_header_has_no_hip_types_and_the_kernels_use_it():
    """The kernels include the very file the model compiles; every probe loop on the device is ds_insert's, bounded by the capacity."""
    src = open(os.path.join(CSRC, "distinct_set.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic", "while (true)", "for (;;)"):
        assert word not in src, word
    assert "for (uint64_t i = 0; i < capacity; i++)" in src and "return DS_OVERFLOW;" in src
    kernels = open(os.path.join(CSRC, "distinct.hip.inc")).read()
    assert '#include "distinct_set.h"' in kernels and '#include "set_walk.h"' in kernels
    for name in ("ds_insert", "ds_key", "ds_word", "ds_bit", "sw_flags16", "sw_codes16", "sw_member"):
        assert name + "(" in kernels, name
    assert "while (" not in kernels and "for (;;)" not in kernels and "goto" not in kernels      # no loop without a bound in its head
    host = open(os.path.join(CSRC, "infidex_hip.hip")).read()
    body = host.split("int32_t infx_field_distinct(")[1].split("int32_t infx_last_field_distinct_info(")[0]
    assert '#include "distinct.hip.inc"' in host and "ds_capacity(ds_max_pairs(" in body and "sts_place_best(" in host.split("static uint32_t dst_place(")[1].split("int32_t infx_field_distinct(")[0]
    for k in ("k_distinct_lds<<<", "k_distinct_bitmap<<<", "k_distinct_hash<<<", "k_distinct_count<<<", "merge_once_shape("):
        assert k in body, k
