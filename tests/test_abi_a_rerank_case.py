"""Registers the contract case of ps_rerank_topk (tests/helpers/abi_cases_rerank.py) in abi_cases' CASES table and runs its
builder's conditions.

The table's readers -- tests/test_abi_cases.py (every stream-taking entry point of the header has a case) and
tests/test_hip_abi_contract.py (the contract matrix) -- parametrise over it when they are collected.  pytest collects a directory's
files in name order and every module before the first test runs, so importing the case module HERE, in a file that sorts before
both, puts the entry point into the table for both whenever the suite, or the directory, is run.  (Either reader run as a
single file does not see this module: name it beside them, e.g. `pytest tests/test_abi_a_rerank_case.py tests/test_abi_cases.py`.)"""
import numpy as np

from helpers import abi_cases as ac
from helpers import abi_cases_rerank as acr  # (the entry point joins ac.CASES)

NAME = "ps_rerank_topk"


def test_this_file_is_collected_before_the_tables_readers():
    assert __name__.rpartition(".")[2] < "test_abi_cases" < "test_hip_abi_contract"
    assert NAME in ac.CASES


def test_builder():
    """tests/test_abi_cases.py::test_builder's conditions, for a run in which that module was collected without this one"""
    c = ac.get(NAME)
    a, b = c.inputs
    assert (acr.N, acr.D, acr.NQ, acr.R, acr.K, acr.ID_OFFSET) == (300, 36, 37, 70, 9, 1000)
    assert all(a[k].tobytes() != b[k].tobytes() for k in a)
    for s in (a, b):
        cand = s["cand"]
        assert cand.shape == (acr.NQ, acr.R) and cand.dtype == np.int64
        rel = cand - acr.ID_OFFSET
        assert (cand == -1).any() and (rel >= acr.N).any() and (rel < 0).any()          # pads and ids outside the table
        assert all(len(set(row.tolist())) < acr.R for row in cand)                      # duplicates
    assert set(c.expect[0]) == {"vals", "ids"}
    assert all(c.expect[0][k].tobytes() != c.expect[1][k].tobytes() for k in c.expect[0])
    assert c.eager_outputs == []                                  # both outputs come from the restatement, bit for bit
    assert c.ws is None and c.workspace_bytes() == 0 and not c.synchronises
    assert sum(v.nbytes for v in a.values()) < 64 << 20
