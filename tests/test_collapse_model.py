"""The arithmetic of Query.collapse_by (infidex_amd/csrc/collapse.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/collapse_model.cpp, which walks k_collapse's steps one after the other — the bitonic network over row indices with its pad indices, the segment
starts, the two exclusive counts — and holds rows, codes, sizes, groups and the list's length to a brute-force fold.

Walked there: every list length in 0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024; one group, all distinct, two alternating, one giant group then singletons,
random with 3, 50 and 4096 codes (the codes 0 and 0xFFFFFFFF among them); keep in 1, 2, 3, 16; a budget of 1, 10, 64 and the list's length.  The stand-alone
program runs plain and under the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

from infidex_amd import Query

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")
WANT = ["OK", str(11 * 7 * 4 * 4)]      # lengths x layouts x keeps x budgets


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp("collapse") / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(HERE, "models", "collapse_model.cpp"), "-o", exe])
    return exe


def run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.split() == WANT, out.stdout


def test_the_steps_equal_a_brute_force_fold(tmp_path_factory):
    run(build(tmp_path_factory, "model", ["-O2"]))
    assert Query("x", collapse_by="shop").collapse_keep == 1      # (the feature this header belongs to)


def test_the_steps_stay_in_their_arrays_under_the_address_sanitizer(tmp_path_factory):
    assert Query("x", collapse_by="shop", collapse_keep=3).collapse_keep == 3
    run(build(tmp_path_factory, "model_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_header_has_no_hip_types_and_the_kernel_includes_it():
    """The kernel includes the very file the model compiles: nothing in it may need the HIP headers."""
    assert Query("x").collapse_by is None
    src = open(os.path.join(CSRC, "collapse.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "__syncthreads", "atomic"):
        assert word not in src, word
    inc = open(os.path.join(CSRC, "collapse.hip.inc")).read()
    assert '#include "collapse.h"' in inc
    for fn in ("clp_before(", "clp_starts(", "clp_segment(", "clp_rank(", "clp_size(", "clp_keeps(", "clp_returned(", "clp_emits("):
        assert fn in inc and fn in src, fn
    hip = open(os.path.join(CSRC, "infidex_hip.hip")).read()
    assert hip.index('#include "fused.hip.inc"') < hip.index('#include "collapse.hip.inc"')      # (wg_bitonic_idx and wg_scan_flags are fused.hip.inc's)
