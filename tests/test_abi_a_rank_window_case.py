"""Registers the contract case of ps_rank_window (tests/helpers/abi_cases_rank_window.py) in abi_cases' CASES table and runs its
builder's conditions.

The table's readers -- tests/test_abi_cases.py (every stream-taking entry point of the header has a case) and
tests/test_hip_abi_contract.py (the contract matrix) -- parametrise over it when they are collected.  pytest collects a directory's
files in name order and every module before the first test runs, so importing the case module HERE, in a file that sorts before
both, puts the entry point into the table for both whenever the suite, or the directory, is run.  (Either reader run as a
single file does not see this module: name it beside them, e.g. `pytest tests/test_abi_a_rank_window_case.py tests/test_abi_cases.py`.)"""
import numpy as np

from helpers import abi_cases as ac
from helpers import abi_cases_rank_window as acr  # (the entry point joins ac.CASES)
from helpers import rank_window_cases as rw

NAME = "ps_rank_window"


def test_this_file_is_collected_before_the_tables_readers():
    assert __name__.rpartition(".")[2] < "test_abi_cases" < "test_hip_abi_contract"
    assert NAME in ac.CASES


def test_builder():
    """tests/test_abi_cases.py::test_builder's conditions, for a run in which that module was collected without this one"""
    c = ac.get(NAME)
    a, b = c.inputs
    assert (acr.S, acr.VP, acr.LD, acr.MAX_TARGET, acr.LO, acr.HI, acr.N_PICKS) == (37, 300, 304, 290, 20, 84, 6)
    assert all(a[k].tobytes() != b[k].tobytes() for k in a)
    for s, e in zip((a, b), c.expect):
        score, skip, u = s["score"], s["skip"], s["u"]
        assert score.shape == (acr.S, acr.LD) and skip.shape == (acr.S,) and u.shape == (acr.S, acr.N_PICKS)
        assert score.dtype == np.float64 and skip.dtype == np.int64 and u.dtype == np.float64
        assert (score[:, acr.MAX_TARGET:] == rw.HUGE).all()                        # beyond max_target and in the pad columns
        # the expectation is the brute-force ranking's
        bw, bn = rw.brute(score, acr.MAX_TARGET, skip, acr.LO, acr.HI)
        assert np.array_equal(e["window"], bw) and np.array_equal(e["nwin"], bn)
        assert np.array_equal(e["picks"], rw.pick(bw, bn, u, acr.N_PICKS))
        assert e["window"].dtype == e["nwin"].dtype == e["picks"].dtype == np.int32
        for r in range(acr.S):                                                     # picks are distinct members of the window
            p = e["picks"][r][e["picks"][r] >= 0]
            assert len(p) == min(acr.N_PICKS, bn[r]) == len(set(p.tolist())) and set(p.tolist()) <= set(bw[r, :bn[r]].tolist())
    assert set(c.expect[0]) == {"window", "nwin", "picks"}
    assert all(c.expect[0][k].tobytes() != c.expect[1][k].tobytes() for k in c.expect[0])
    assert c.eager_outputs == []                                  # every output comes from the restatement, bit for bit
    assert c.ws is None and not c.synchronises
    assert sum(v.nbytes for v in a.values()) < 64 << 20
