"""The member walk of bucket_stats (infidex_amd/csrc/bucket_stats.h on range_buckets.h and exact_sum.h) without a GPU: the three headers, UNCHANGED, compiled
with g++ into tests/models/bucket_stats_model.cpp, which sends random members through bks_member into slots laid out as the kernel lays them out, from one
thread and from eight, and holds every slot's counters, extreme ranks and recombined sum to a brute-force scan on __int128 that never looks at a threshold
search, a limb or a scale.

Walked there: 1, 2, 8, 255 and 256 buckets; runs of equal thresholds (empty buckets), thr[0] at its floor and thr[B] = the number of values; nanRanks 0 and
1; value tables of one to four limbs, int64 with both extremes and doubles with NaN, +-inf and +-0.0.  The program has its own main and runs plain and under
the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

import pytest

from infidex_amd import BucketStatsRequest      # (the feature these headers belong to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def model(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bucket_stats_" + request.param) / "bucket_stats_model")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    # -Wno-unknown-pragmas: the headers' `#pragma unroll` is the kernels'
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread", *flags,
                           "-I", CSRC, os.path.join(HERE, "models", "bucket_stats_model.cpp"), "-o", exe])
    return exe


def test_every_slot_equals_a_brute_force_scan(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    # cases (7 tables x 5 bucket counts x 2 nanRanks x 4 shapes x {1, 8} threads, and two more), members walked, slots held, empty slots, slots with both infinities
    assert f[0] == "OK" and int(f[1]) == 7 * 5 * 2 * 4 * 2 + 2 and int(f[2]) > 500000 and int(f[4]) > 10000 and int(f[5]) > 100, out.stdout
    assert int(f[3]) == 7 * 2 * 4 * 2 * sum(b + 3 for b in (1, 2, 8, 255, 256)) + 4 + 5, out.stdout      # B + 3 slots per request
    assert BucketStatsRequest().bucket_by is None


def test_the_header_has_no_hip_types_and_reuses_the_bucket_and_sum_arithmetic():
    """The kernel includes the very file the model compiles; the slot is rb_slot's and the limbs are xs_limbs', not copies of them, and neither header changed
    for it."""
    src = open(os.path.join(CSRC, "bucket_stats.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic"):
        assert word not in src, word
    assert '#include "range_buckets.h"' in src and '#include "exact_sum.h"' in src
    for name in ("rb_slot", "xs_limbs", "rb_slots"):
        assert name + "(" in src and "uint32_t %s(" % name not in src, name
    for name in ("rb_upper_bound", "xs_unpack"):                                     # what those two are made of is not restated
        assert name not in src, name
    kernels = open(os.path.join(CSRC, "bucket_stats.hip.inc")).read()
    assert '#include "bucket_stats.h"' in kernels
    for name in ("bks_member", "sw_flags16", "sts_values16", "sw_codes16", "sts_add", "sts_stride"):
        assert name + "(" in kernels, name
    code = "\n".join(line.split("//")[0] for line in kernels.split('#include "bucket_stats.h"')[1].splitlines())
    for word in ("float", "double", "atomicCAS", "atomicExch", "atomicInc", "atomicSub"):      # integers only, and no atomic that decides a position
        assert word not in code, word
    host = open(os.path.join(CSRC, "infidex_hip.hip")).read()
    body = host.split("int32_t infx_bucket_stats(")[1].split("int32_t infx_last_bucket_stats_info(")[0]
    assert '#include "bucket_stats.hip.inc"' in host and "k_bucket_stats<<<" in body and "sts_place_best(" in body and "set_fetch_raw(" in body
    assert body.count("k_bucket_stats<<<") == 1                                      # one launch for all requests of a call
