"""Registers the contract cases of ps_walk_paths_biased and ps_paths_topk (tests/helpers/abi_cases_biased.py) in abi_cases' CASES
table and runs their builders' conditions.

The table's readers -- tests/test_abi_cases.py (every stream-taking entry point of the header has a case) and
tests/test_hip_abi_contract.py (the contract matrix) -- parametrise over it when they are collected.  pytest collects a directory's
files in name order and every module before the first test runs, so importing the case module HERE, in a file that sorts before
both, puts the entry points into the table for both whenever the suite, or the directory, is run."""
import numpy as np
import pytest

from helpers import abi_cases as ac
from helpers import abi_cases_biased as acb  # (the entry points join ac.CASES)

NAMES = ("ps_walk_paths_biased", "ps_paths_topk")


def test_this_file_is_collected_before_the_tables_readers():
    assert __name__.rpartition(".")[2] < "test_abi_cases" < "test_hip_abi_contract"
    assert all(n in ac.CASES for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_builder(name):
    """tests/test_abi_cases.py::test_builder's conditions, for a run in which that module was collected without this one"""
    c = ac.get(name)
    a, b = c.inputs
    assert any(a[k].tobytes() != b[k].tobytes() for k in a)
    assert all(c.expect[0][k].tobytes() != c.expect[1][k].tobytes() for k in c.expect[0])
    assert c.eager_outputs == []                                  # every output comes from the restatement, bit for bit
    assert c.ws is None and c.workspace_bytes() == 0 and not c.synchronises
    assert sum(v.nbytes for v in a.values()) < 64 << 20


def test_the_walk_case_stands_on_every_degree_with_a_previous_node():
    from helpers import biased_walk_cases as bc
    _, _, V, info, adj, _ = bc.case_graph(True)
    deg = np.array([len(r) for r in adj])
    for s in ac.get("ps_walk_paths_biased").expect:
        paths = s["paths"]
        stood = paths[:, :-1][paths[:, 1:] >= 0]                  # nodes a step was taken FROM after the first
        assert set(bc.DEGREES) <= set(deg[stood].tolist())
