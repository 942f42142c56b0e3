"""The lowering of a filter leaf over a list column without a GPU: host/filter.h and host/list_columns.h, UNCHANGED, compiled with g++ into
tests/models/list_columns_model.cpp, which does what k_list_leaf does with their output (its header comment).  For each of the 13 LeafOps over int, double
and string element dictionaries the derived bit of every document equals the OR of leaf_holds over its elements, and leaf_holds of a null value for an empty
list.  The same program is built and run with -fsanitize=address,undefined: a host program with its own main."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "list_columns_model.cpp")
OPS = ["EQ", "GT", "GE", "LT", "LE", "BETWEEN", "IN", "CONTAINS", "STARTS", "ENDS", "LIKE", "ISNULL", "NOTNULL"]      # filter.h's LeafOp, in order


def build_and_run(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", *flags, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    text = build_and_run(tmp_path_factory.mktemp("list_columns"), "list_columns_model", [])
    return [[int(x) for x in line.split()] for line in text.splitlines()]


def test_every_operator_and_kind_matches_the_any_element_rule(rows):
    assert len(rows) == 3 * 13
    assert [(r[0], r[1]) for r in rows] == [(k, o) for k in (1, 2, 3) for o in range(13)]
    for kind, op, docs, hits, empty, mism in rows:
        assert mism == 0, (kind, OPS[op])
        assert docs == 211
        assert 0 < hits < docs, (kind, OPS[op], hits)                     # no leaf of the model is constant over the documents


def test_an_empty_list_is_a_null_value(rows):
    """leaf_holds of a null value decides an empty list: IS NULL holds, and so do < and <= (FilterVM orders a null below every constant, for a scalar field
    too); =, >, >=, BETWEEN, IN and IS NOT NULL do not.  CONTAINS, STARTS WITH, ENDS WITH and LIKE read a null as the empty string, which the model's
    constants do not match."""
    for kind, op, _, _, empty, _ in rows:
        assert empty == (1 if OPS[op] in ("ISNULL", "LT", "LE") else 0), (kind, OPS[op])


def test_is_null_counts_the_empty_lists(rows):
    """211 documents of which the first, the last, a run of twenty and every sixth are empty: over ints and doubles IS NULL and IS NOT NULL split them.
    Only the string dictionary holds an empty-string element, which IS NULL accepts as well: a list with "" and another value is in both."""
    by = {(r[0], OPS[r[1]]): r for r in rows}
    for kind in (1, 2):
        assert by[(kind, "ISNULL")][3] + by[(kind, "NOTNULL")][3] == 211
    assert by[(1, "ISNULL")][3] == by[(2, "ISNULL")][3] < by[(3, "ISNULL")][3]
    assert by[(3, "ISNULL")][3] + by[(3, "NOTNULL")][3] > 211


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    text = build_and_run(tmp_path, "list_columns_model_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert len(text.splitlines()) == 39 and all(line.split()[-1] == "0" for line in text.splitlines())
