"""The ranking of top_groups (infidex_amd/csrc/top_select.h on listing_select.h and exact_sum.h) without a GPU: the three headers, UNCHANGED, compiled with
g++ into tests/models/top_select_model.cpp, which builds every group's composite and walks the whole multi-word select serially the way k_top_keys,
k_top_hist, k_top_pick, k_top_gather and k_top_page do, and compares every page row for row with std::sort under an exact comparator that never looks at a
composite: the class, the figure as a typed value (unsigned, 128-bit integer, double), the tie.

Walked there: random tables and tables whose keys are all equal; 1, 2, 7, 100 and 2049 groups; every `by` in both directions; doubles with +-0.0,
subnormals, +-inf and NaN; int sums at -2^127 and 2^127 - 1 and around +-2^64; groups with no member and groups without a figure; offsets at 0, inside a
tie run, at total_groups - 1 and beyond; digit widths 4 and 11 and one between.  The program runs under the address and undefined-behaviour sanitizers (host
code with its own main)."""
import os
import subprocess

import pytest

from infidex_amd import TopGroupsRequest      # (the feature these headers belong to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_select") / "top_select_model")
    # -Wno-unknown-pragmas: the headers' `#pragma unroll` is the kernels'
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(HERE, "models", "top_select_model.cpp"), "-o", exe])
    return exe


def test_every_page_equals_a_plain_sort_under_an_exact_comparator(model):
    out = subprocess.run([model], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    f = out.stdout.split()
    # pages, rows compared, pages that begin inside a tie run, groups without a figure, groups without a member, empty pages
    assert f[0] == "OK" and int(f[1]) > 50000 and int(f[2]) > 1000000 and int(f[3]) > 1000 and int(f[4]) > 1000 and int(f[5]) > 1000 and int(f[6]) > 1000, out.stdout
    assert TopGroupsRequest().by == "size"


def test_headers_have_no_hip_types_and_reuse_the_listing_and_sum_arithmetic():
    """The kernels include the very file the model compiles; the digit picking is listing_select.h's and the sums are exact_sum.h's, not copies of them."""
    src = open(os.path.join(CSRC, "top_select.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomic"):
        assert word not in src, word
    assert '#include "listing_select.h"' in src and '#include "exact_sum.h"' in src
    for name in ("ls_pick", "xs_recombine", "xs_sum_bits", "xs_mean_bits", "xs_sum_int128"):
        assert name + "(" in src and "uint32_t %s(" % name not in src and "bool %s(" % name not in src and "uint64_t %s(" % name not in src, name
    kernels = open(os.path.join(CSRC, "top_groups.hip.inc")).read()
    assert '#include "top_select.h"' in kernels
    for name in ("ts_figure", "ts_compose", "ts_digit", "ts_under_prefix", "ts_start", "ts_step", "ts_on_page", "ts_cmp", "sw_flags16", "sw_codes16", "sw_member"):
        assert name + "(" in kernels, name
    host = open(os.path.join(CSRC, "infidex_hip.hip")).read()
    assert '#include "top_groups.hip.inc"' in host and "k_field_stats<<<" in host.split("int32_t infx_top_groups(")[1].split("int32_t infx_last_top_groups_info(")[0]
