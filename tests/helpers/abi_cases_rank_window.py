"""The case of the contract matrix (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py) for the rank-window select,
csrc/rank_window.hip: ps_rank_window.  All three outputs are held to rank_window_cases' restatement bit for bit (no eager
expectation); the entry point takes no workspace and does not synchronise.

The builder is written exactly as abi_cases' own and joins its CASES table through its `case` decorator when this module is
imported; tests/test_abi_a_rank_window_case.py imports it, and is collected before the test modules that read the table;
tests/test_hip_rank_window.py imports it too and starts the contract matrix for the entry point itself."""
import functools

import numpy as np

from helpers import abi_cases as ac
from helpers.abi_cases import I, O, ST, Case, _c

S, VP, LD, MAX_TARGET, LO, HI, N_PICKS = 37, 300, 304, 290, 20, 84, 6


@functools.lru_cache(maxsize=None)
def _sets():
    """two score matrices of 37 rows and their restated outputs: full rows, rows that end inside the window and ahead of it, a
    row of zeros, tie groups over either boundary, junk that never competes, huge scores beyond max_target and in the pad
    columns, skip entries inside and outside [0, limit)"""
    from helpers import rank_window_cases as rw
    out = []
    for seed in (1, 2):
        rs = np.random.RandomState(8900 + seed)
        score = np.full((S, LD), rw.HUGE, np.float64)
        for s in range(S):
            N = (MAX_TARGET, 0, 50, LO, 200, LO + 3, HI, 120)[(s + seed) % 8]
            keys = rw.distinct_keys(rs, N)
            if N > HI:
                keys = rw.tie(keys, LO - 2, LO + 3) if s % 2 else rw.tie(keys, HI - 3, HI + 2)
            score[s, :VP] = rw.row_from_keys(rs, VP, MAX_TARGET, keys, salt=True)
        skip = rs.randint(0, MAX_TARGET, S).astype(np.int64)
        skip[seed::9] = [-1, MAX_TARGET, VP + 1, 1 << 40][:len(skip[seed::9])]
        u = rs.random_sample((S, N_PICKS))
        u[seed] = 0.0
        window, nwin = rw.restate(score, MAX_TARGET, skip, LO, HI)
        picks = rw.pick(window, nwin, u, N_PICKS)
        assert (nwin == HI - LO).any() and (nwin == 0).any() and ((nwin > 0) & (nwin < N_PICKS)).any()
        assert ((skip >= 0) & (skip < MAX_TARGET)).any() and (skip < 0).any() and (skip >= MAX_TARGET).any()
        assert (picks == -1).any() and (picks >= 0).any() and np.isnan(score[:, :MAX_TARGET]).any()
        out.append((dict(score=_c(score), skip=_c(skip), u=_c(u)), dict(window=window, nwin=nwin, picks=picks)))
    return tuple(out)


@ac.case
def _ps_rank_window(name):
    sets = _sets()
    return Case(name, [I("score"), S, LD, VP, MAX_TARGET, I("skip"), LO, HI, I("u"), N_PICKS, O("window"), O("nwin"), O("picks"), ST],
                tuple(s[0] for s in sets),
                {"window": ((S, HI - LO), np.int32), "nwin": ((S,), np.int32), "picks": ((S, N_PICKS), np.int32)},
                tuple(s[1] for s in sets))
