"""Registers the contract cases of ps_layer_norm and ps_layer_norm_bwd (tests/helpers/abi_cases_layer_norm.py) in abi_cases' CASES
table and runs their builders' conditions.

The table's readers -- tests/test_abi_cases.py (every stream-taking entry point of the header has a case) and
tests/test_hip_abi_contract.py (the contract matrix) -- parametrise over it when they are collected.  pytest collects a directory's
files in name order and every module before the first test runs, so importing the case module HERE, in a file that sorts before
both, puts the two entry points into the table for both whenever the suite, or the directory, is run.  (Either reader run as a
single file does not see this module: name it beside them, e.g. `pytest tests/test_abi_a_layer_norm_case.py tests/test_abi_cases.py`.)"""
import pytest

from helpers import abi_cases as ac
from helpers import abi_cases_layer_norm  # noqa: F401  (the two entry points join ac.CASES)

OUTPUTS = {"ps_layer_norm": {"y", "mean", "rstd"}, "ps_layer_norm_bwd": {"gx", "dgamma", "dbeta"}}


def test_this_file_is_collected_before_the_tables_readers():
    assert __name__.rpartition(".")[2] < "test_abi_cases" < "test_hip_abi_contract"
    assert set(OUTPUTS) <= set(ac.CASES)


@pytest.mark.parametrize("name", sorted(OUTPUTS))
def test_builder(name):
    """tests/test_abi_cases.py::test_builder's conditions, for a run in which that module was collected without this one"""
    c = ac.get(name)
    a, b = c.inputs
    assert any(a[k].tobytes() != b[k].tobytes() for k in a)
    assert "live" in a and (a["live"] <= 0).any() and (a["live"] > 0).any()           # with a mask
    assert set(c.expect[0]) == OUTPUTS[name]
    assert all(c.expect[0][k].tobytes() != c.expect[1][k].tobytes() for k in c.expect[0])
    assert c.eager_outputs == []                                  # every output comes from the restatement, bit for bit
    assert not c.synchronises
    if name == "ps_layer_norm_bwd":                               # the forward takes no workspace
        assert c.workspace_bytes() > 0
    assert sum(v.nbytes for v in a.values()) < 64 << 20
