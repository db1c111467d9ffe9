"""Registers the contract case of ps_bn_bwd (tests/helpers/abi_cases_bn_bwd.py) in abi_cases' CASES table and runs its builder's
conditions.

The table's readers -- tests/test_abi_cases.py (every stream-taking entry point of the header has a case) and
tests/test_hip_abi_contract.py (the contract matrix) -- parametrise over it when they are collected.  pytest collects a directory's
files in name order and every module before the first test runs, so importing the case module HERE, in a file that sorts before
both, puts ps_bn_bwd into the table for both whenever the suite, or the directory, is run.  (Either reader run as a single file
does not see this module: name it beside them, e.g. `pytest tests/test_abi_bn_bwd_case.py tests/test_abi_cases.py`.)"""
from helpers import abi_cases as ac
from helpers import abi_cases_bn_bwd  # noqa: F401  (ps_bn_bwd joins ac.CASES)

NAME = "ps_bn_bwd"


def test_this_file_is_collected_before_the_tables_readers():
    assert __name__.rpartition(".")[2] < "test_abi_cases" < "test_hip_abi_contract"
    assert NAME in ac.CASES


def test_builder():
    """tests/test_abi_cases.py::test_builder's conditions, for a run in which that module was collected without this one"""
    c = ac.get(NAME)
    a, b = c.inputs
    assert any(a[k].tobytes() != b[k].tobytes() for k in a)
    assert set(c.expect[0]) == {"gz", "dgamma", "dbeta"}
    assert all(c.expect[0][k].tobytes() != c.expect[1][k].tobytes() for k in c.expect[0])
    assert c.eager_outputs == []                                  # every output comes from the restatement, bit for bit
    assert c.workspace_bytes() > 0 and not c.synchronises
    assert sum(v.nbytes for v in a.values()) < 64 << 20
