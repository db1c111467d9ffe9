"""Registers the contract case of ps_frontier_build (tests/helpers/abi_cases_frontier.py) in abi_cases' CASES table and runs its
builder's conditions.

The table's readers -- tests/test_abi_cases.py (every stream-taking entry point of the header has a case) and
tests/test_hip_abi_contract.py (the contract matrix) -- parametrise over it when they are collected.  pytest collects a directory's
files in name order and every module before the first test runs, so importing the case module HERE, in a file that sorts before
both, puts the entry point into the table for both whenever the suite, or the directory, is run.  (Either reader run as a
single file does not see this module: name it beside them, e.g. `pytest tests/test_abi_a_frontier_case.py tests/test_abi_cases.py`.)"""
import numpy as np

from helpers import abi_cases as ac
from helpers import abi_cases_frontier as acf  # (the entry point joins ac.CASES)
from helpers import frontier_cases as fc

NAME = "ps_frontier_build"


def test_this_file_is_collected_before_the_tables_readers():
    assert __name__.rpartition(".")[2] < "test_abi_cases" < "test_hip_abi_contract"
    assert NAME in ac.CASES


def test_builder():
    """tests/test_abi_cases.py::test_builder's conditions, for a run in which that module was collected without this one"""
    c = ac.get(NAME)
    a, b = c.inputs
    assert (acf.S, acf.B, acf.T, acf.LIMIT, acf.ROOM) == (40, 37, 6, 300, 262)
    assert all(a[k].tobytes() != b[k].tobytes() for k in a)
    for s, e in zip((a, b), c.expect):
        seeds, ids, nvalid = s["seeds"], s["ids"], s["nvalid"]
        assert seeds.shape == (acf.S,) and ids.shape == (acf.B, acf.T) and nvalid.shape == (acf.B,)
        assert all(t.dtype == np.int32 for t in (seeds, ids, nvalid))
        assert len(set(seeds.tolist())) == acf.S and seeds.min() >= 0 and seeds.max() < acf.LIMIT      # the seeds' contract
        assert (ids < 0).any() and (ids >= acf.LIMIT).any() and (nvalid < 0).any() and (nvalid > acf.T).any()
        # the expectation is the brute-force set definition's, and the canary behind it
        n = int(e["count"][0])
        bf, bl = fc.brute(seeds, ids, nvalid, acf.T, acf.LIMIT)
        assert acf.S < n < acf.ROOM and np.array_equal(e["frontier"][:n], bf) and np.array_equal(e["local"], bl)
        assert np.all(e["frontier"][n:] == acf.CANARY) and e["frontier"][n:].tobytes() == b"\xff" * (4 * (acf.ROOM - n))
    assert set(c.expect[0]) == {"frontier", "count", "local"}
    assert all(c.expect[0][k].tobytes() != c.expect[1][k].tobytes() for k in c.expect[0])
    assert c.eager_outputs == []                                  # every output comes from the restatement, bit for bit
    assert c.ws is not None and not c.synchronises
    assert c.workspace_bytes() >= 2 * 4096 + 4 * acf.LIMIT      # two bitmaps of one scan block, the map
    assert sum(v.nbytes for v in a.values()) < 64 << 20
