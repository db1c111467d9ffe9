"""The case of the contract matrix (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py) for the set operation behind a
minibatch block, csrc/frontier.hip: ps_frontier_build.  All three outputs are held to frontier_cases.restate bit for bit (no eager
expectation); the entry point takes a workspace and does not synchronise.

`frontier` is a buffer of S + min(B * T, limit) entries of which the call writes the first count[0] and leaves the rest untouched.
The contract matrix fills every output with 0xFF bytes before a call, so the expectation is the restated frontier followed by that
canary (int32 -1) up to the buffer's end: one byte comparison holds the order of the written part and the untouched tail.

The builder is written exactly as abi_cases' own and joins its CASES table through its `case` decorator when this module is
imported; tests/test_abi_a_frontier_case.py imports it, and is collected before the test modules that read the table;
tests/test_hip_minibatch.py imports it too and starts the contract matrix for the entry point itself."""
import functools

import numpy as np

from helpers import abi_cases as ac
from helpers.abi_cases import I, O, ST, WS, WSB, Case, _c

S, B, T, LIMIT = 40, 37, 6, 300
ROOM = S + min(B * T, LIMIT)              # entries of `frontier`
CANARY = np.int32(-1)                     # four 0xFF bytes: what the contract matrix fills an output with


@functools.lru_cache(maxsize=None)
def _sets():
    """two input sets and their restated outputs: 40 seeds in no order, 37 rows of 6 slots (B != S, 222 slots: one ragged
    workgroup beside the seeds'), ids on either side of [0, limit), -1 pads, rows with nvalid 0, below 0 and above T, slots behind
    nvalid that hold in-range ids, seeds among the neighbours and ids shared by several rows"""
    from helpers import frontier_cases as fc
    out = []
    for seed in (1, 2):
        rs = np.random.RandomState(8800 + seed)
        seeds = rs.permutation(LIMIT)[:S].astype(np.int32)
        ids = rs.randint(0, LIMIT // (2 * seed), (B, T)).astype(np.int32)      # a narrow range: ids shared by several rows
        nvalid = rs.randint(1, T + 1, B).astype(np.int32)
        ids[::5, 1] = LIMIT
        ids[1::5, 2] = -1
        ids[2::7, 0] = seeds[:len(ids[2::7])]
        ids[3, :] = [LIMIT - 1, LIMIT + 7, -7, 0, seeds[5], LIMIT - 1]
        nvalid[[3, 4, 9, 11, 20]] = [T, 0, -3, T + 4, 0]
        frontier, local = fc.restate(seeds, ids, nvalid, T, LIMIT)
        keep = fc.kept_mask(ids, nvalid, T, LIMIT)
        assert keep.any() and (~keep).any() and (ids[keep][:, None] == seeds[None, :]).any()
        behind = ids[np.arange(T)[None, :] >= np.clip(nvalid, 0, T)[:, None]]
        assert ((behind >= 0) & (behind < LIMIT)).any()
        assert len(np.unique(ids[keep])) < keep.sum()                          # an id in several slots
        assert S < len(frontier) < ROOM                                        # something emitted, and a tail left over
        full = np.full(ROOM, CANARY, np.int32)
        full[:len(frontier)] = frontier
        out.append((dict(seeds=_c(seeds), ids=_c(ids), nvalid=_c(nvalid)),
                    dict(frontier=full, count=np.array([len(frontier)], np.int32), local=local)))
    assert out[0][1]["count"][0] != out[1][1]["count"][0]
    return tuple(out)


@ac.case
def _ps_frontier_build(name):
    sets = _sets()
    return Case(name, [I("seeds"), S, I("ids"), I("nvalid"), B, T, LIMIT, O("frontier"), O("count"), O("local"), WS, WSB, ST],
                tuple(s[0] for s in sets),
                {"frontier": ((ROOM,), np.int32), "count": ((1,), np.int32), "local": ((B, T), np.int32)},
                tuple(s[1] for s in sets), ws=("ps_frontier_workspace_bytes", (LIMIT, S, B, T)))
