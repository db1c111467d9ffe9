"""The case of the contract matrix (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py) for the second level of the two-level
search, csrc/rerank.hip: ps_rerank_topk.  Both outputs are held to rerank_cases.restate bit for bit (no eager expectation); the
entry point takes no workspace and does not synchronise.

The builder is written exactly as abi_cases' own and joins its CASES table through its `case` decorator when this module is
imported; tests/test_abi_a_rerank_case.py imports it, and is collected before the test modules that read the table;
tests/test_hip_rerank.py imports it too and starts the contract matrix for the entry point itself."""
import functools

import numpy as np

from helpers import abi_cases as ac
from helpers.abi_cases import I, O, ST, Case, _c

N, D, NQ, R, K, ID_OFFSET = 300, 36, 37, 70, 9, 1000


@functools.lru_cache(maxsize=None)
def _sets():
    """two input sets and their restated outputs: D = 36 (16-byte loads, a full tile of 32 columns and one of 4), R = 70 (two
    lane rounds), 37 queries (a ragged last workgroup); the lists hold -1 pads, ids on either side of the table's range, a plain
    row index (below the offset) and duplicates; row 5 has fewer than K valid candidates, row 6 none"""
    from helpers import rerank_cases as rc
    out = []
    for seed in (1, 2):
        rs = np.random.RandomState(7700 + seed)
        E = rs.standard_normal((N, D)).astype(np.float32)
        Q = rs.standard_normal((NQ, D)).astype(np.float32)
        cand = np.stack([rs.permutation(N)[:R] for _ in range(NQ)]).astype(np.int64) + ID_OFFSET
        cand[:, 3 + seed] = -1
        cand[::2, 40] = ID_OFFSET + N
        cand[1::2, 41] = ID_OFFSET - 1
        cand[::3, 66] = 17
        cand[:, 69] = cand[:, 0]
        cand[::4, 30:34] = cand[::4, 10:14]
        cand[5, 4:] = -1
        cand[6, :] = [-1, ID_OFFSET + N, 5, -9, ID_OFFSET - 1] * (R // 5)
        vals, ids = rc.restate(E, Q, cand, K, ID_OFFSET)
        assert (cand == -1).any() and (cand >= ID_OFFSET + N).any() and ((cand >= 0) & (cand < ID_OFFSET)).any()
        assert all(len(set(row.tolist())) < R for row in cand)                          # a duplicate in every list
        assert (ids[5] >= 0).sum() == 4 and (ids[6] == -1).all() and np.isneginf(vals[6]).all() and (ids[:5] >= ID_OFFSET).all()
        out.append((dict(E=_c(E), Q=_c(Q), cand=_c(cand)), dict(vals=vals, ids=ids)))
    return tuple(out)


@ac.case
def _ps_rerank_topk(name):
    sets = _sets()
    return Case(name, [I("E"), N, D, ID_OFFSET, I("Q"), NQ, I("cand"), R, K, O("vals"), O("ids"), ST], tuple(s[0] for s in sets),
                {"vals": ((NQ, K), np.float32), "ids": ((NQ, K), np.int64)}, tuple(s[1] for s in sets))
