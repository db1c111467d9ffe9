"""The cases of the contract matrix (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py) for csrc/walk_biased.hip
(ps_walk_paths_biased) and csrc/walk_topk.hip (ps_paths_topk).  Every output is held to tests/helpers/biased_walk_cases.py bit for bit (no eager
expectation); neither entry point takes a workspace or synchronises.

The builders join abi_cases' CASES table through its `case` decorator when this module is imported;
tests/test_abi_a_biased_walk_case.py imports it, and is collected before the test modules that read the table."""
import functools

import numpy as np

from helpers import abi_cases as ac
from helpers import biased_walk_cases as bc
from helpers.abi_cases import I, O, ST, Case, _c

L = 3
BIAS = ((0.25, 4.0), (4.0, 0.25))                # (p, q) of the two input sets
W_TOPK, L_TOPK, T_TOPK = 21, 3, 10


@functools.lru_cache(maxsize=None)
def _walk_sets():
    """the case graph WITH sinks (paths end in -1), every node a start, plus starts outside the graph; the stream mode with one
    position per walk.  The two sets share the graph and differ in starts, uniforms and bias."""
    ei, w, V, info, adj, outs = bc.case_graph(True)
    rowptr, col, wsorted, cdf, nbr = bc.host_csr(ei, w, V)
    out = []
    for k, (p, q) in enumerate(BIAS):
        rs = np.random.RandomState(4100 + k)
        starts = np.concatenate([rs.permutation(V), rs.randint(0, V, size=V // 2), [-1, V, V + 7, 2 ** 40]]).astype(np.int64)
        B = starts.size
        u = rs.random_sample(B * L)
        uoff = rs.permutation(B).astype(np.int64) * L
        paths = np.stack([bc.replay_walk(adj, outs, int(s), L, u, int(o), 1.0 / p, 1.0 / q) for s, o in zip(starts, uoff)])
        assert (paths[:, -1] >= 0).any() and (paths[:, 0] < 0).any() and ((paths[:, 0] >= 0) & (paths[:, -1] < 0)).any()
        ins = dict(rowptr=_c(rowptr), col=_c(col), wsorted=_c(wsorted), cdf=_c(cdf), nbr=_c(nbr), starts=_c(starts), uniforms=_c(u),
                   uoff=_c(uoff), bias=_c(np.array([1.0 / p, 1.0 / q])))
        out.append((ins, dict(paths=paths)))
    return V, tuple(out)


@ac.case
def _ps_walk_paths_biased(name):
    from pinsage_hip import native as nv
    V, sets = _walk_sets()
    B = sets[0][0]["starts"].size
    return Case(name, [I("rowptr"), I("col"), I("wsorted"), I("cdf"), I("nbr"), V, I("starts"), B, L, nv.PS_RNG_STREAM, I("uniforms"),
                       I("uoff"), 0, 0, 0, I("bias"), O("paths"), ST], tuple(s[0] for s in sets), {"paths": ((B, L), np.int32)},
                tuple(s[1] for s in sets))


@functools.lru_cache(maxsize=None)
def _topk_sets():
    """70 rows of W * L = 63 entries over few ids (many repeats and ties), with -1 holes; row 3 is empty, row 4 holds one id, row
    5 all different ids (all counts equal: first-visit order decides), row 6 fewer than T ids (three, two in the second set)"""
    n = W_TOPK * L_TOPK
    out = []
    for seed in (1, 2):
        rs = np.random.RandomState(5200 + seed)
        paths = rs.randint(0, 12 + 10 * seed, size=(70, n)).astype(np.int32)
        paths[rs.random_sample(paths.shape) < 0.15] = -1
        paths[3] = -1
        paths[4] = 77
        paths[5] = rs.permutation(1000)[:n]
        paths[6] = np.resize([5, -1, 9, 5, 2][:6 - seed], n)
        ids, counts, nvalid = bc.topk_from_paths(paths, T_TOPK)
        assert nvalid[3] == 0 and nvalid[4] == 1 and nvalid[6] == 4 - seed and (nvalid == T_TOPK).any()
        assert ids[5].tolist() == paths[5, :T_TOPK].tolist() and (counts[5] == 1).all()
        out.append((dict(paths=_c(paths)), dict(ids=ids, counts=counts, nvalid=nvalid)))
    return tuple(out)


@ac.case
def _ps_paths_topk(name):
    sets = _topk_sets()
    n = W_TOPK * L_TOPK
    return Case(name, [I("paths"), 70, n, T_TOPK, O("ids"), O("counts"), O("nvalid"), ST], tuple(s[0] for s in sets),
                {"ids": ((70, T_TOPK), np.int32), "counts": ((70, T_TOPK), np.int32), "nvalid": ((70,), np.int32)},
                tuple(s[1] for s in sets))
