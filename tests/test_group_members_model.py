"""The arithmetic of list_group_members' walk (infidex_amd/csrc/group_members.h) without a GPU: the header, UNCHANGED, compiled with g++ into
tests/models/group_members_model.cpp, where gm_insert works on std::atomic slots whose minimum is a compare-and-swap loop — the kernels pass the 64-bit
minimum of the LDS and of global memory instead — and every run's slots are held to std::sort, slot by slot, the empty ones behind.

Walked there: every permutation of seven composites (keys shared by two) into 1 .. 4 slots; random streams of 0, 1, N-1, N, N+1 and 5000 composites with 1, 3
and 50 distinct keys for N in {1, 2, 3, 7, 16}; eight threads feeding one row, and the kernel's two levels — four groups of two threads with a table each,
merged into a shared table by the same gm_insert while the other groups still insert — for N in {1, 2, 3, 4, 7, 16}.  The stand-alone program runs plain,
under the thread sanitizer and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from infidex_amd import GroupMembersRequest      # (the feature this header belongs to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "infidex_amd", "csrc")
# 4 x 7! permutation runs; 5 N x 6 lengths x 3 key counts; 6 N x 6 lengths x 2 key counts, flat and in two levels
WANT = ["OK", str(4 * 5040), str(5 * 6 * 3), str(6 * 6 * 2), str(6 * 6 * 2)]


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp("group_members") / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *flags, "-I", CSRC, os.path.join(HERE, "models", "group_members_model.cpp"), "-o", exe])
    return exe


def run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.split() == WANT, out.stdout


def test_slots_are_the_smallest_composites_in_order_from_one_thread_and_from_eight(tmp_path_factory):
    run(build(tmp_path_factory, "model", ["-O2"]))
    assert GroupMembersRequest().per_group == 3


def test_the_walk_is_race_free_under_the_thread_sanitizer(tmp_path_factory):
    run(build(tmp_path_factory, "model_tsan", ["-O1", "-g", "-fsanitize=thread"]))


def test_the_walk_stays_in_its_slots_under_the_address_sanitizer(tmp_path_factory):
    run(build(tmp_path_factory, "model_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_header_has_no_hip_types_and_the_kernels_include_it():
    """The kernels include the very file the model compiles: nothing in it may need the HIP headers, and the minimum is the includer's."""
    src = open(os.path.join(CSRC, "group_members.h")).read()
    for word in ("hip/", "uint4", "threadIdx", "blockIdx", "__shfl", "__global__", "__shared__", "atomicMin", "__hip_atomic"):
        assert word not in src, word
    inc = open(os.path.join(CSRC, "group_members.hip.inc")).read()
    assert '#include "group_members.h"' in inc and "gm_insert(GmLdsSlots" in inc and "gm_insert(GmGlobalSlots" in inc
    hip = open(os.path.join(CSRC, "infidex_hip.hip")).read()
    assert hip.index('#include "groups.hip.inc"') < hip.index('#include "group_members.hip.inc"')
    assert "atomic" not in open(os.path.join(CSRC, "group_heads.h")).read()      # (the slot walk did not go into the heads' header)
