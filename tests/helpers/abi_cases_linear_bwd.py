"""The cases of the contract matrix (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py) for the dense layers' backward,
csrc/linear_bwd.hip: ps_linear_wgrad and ps_linear_epilogue_bwd.  Every output of both is held to linear_bwd_cases' numpy
restatement bit for bit (no eager expectation).

The builders are written exactly as abi_cases' own and join its CASES table through its `case` decorator when this module is
imported; tests/helpers/__init__.py imports it, so the table is complete before any test module reads it."""
import numpy as np

from helpers import abi_cases as ac
from helpers.abi_cases import I, O, WS, WSB, ST, Case, _c


@ac.case
def _ps_linear_wgrad(name):
    """two partitions (M > P): the workspace and both launches; 16-byte sweeps; dW and db bit for bit"""
    from helpers import linear_bwd_cases as lb
    N, K = 36, 24
    M = lb.partition(1) + 70
    P = lb.partition(M)
    assert M > P and lb.partition_rule(M) == P
    ins, exp = [], []
    for seed in (1, 2):
        g, x = lb.wgrad_data(M, N, K, P, seed=seed)
        ins.append({"g": _c(g), "x": _c(x)})
        exp.append({"dW": lb.wgrad_exact(g, x, P), "db": lb.bias_grad_exact(g, P)})
    return Case(name, [I("g"), M, N, I("x"), K, O("dW"), O("db"), WS, WSB, ST], tuple(ins),
                {"dW": ((N, K), np.float32), "db": ((N,), np.float32)}, tuple(exp), ws=("ps_linear_wgrad_workspace_bytes", (M, N, K)))


@ac.case
def _ps_linear_epilogue_bwd(name):
    """ReLU and row norm, N = 300: 16-byte sweeps, rows longer than one sweep; the planted zero and near-clamp rows included,
    the NaN row not (the comparison is of bytes, and a NaN's payload is nobody's contract)"""
    from helpers import linear_bwd_cases as lb
    from pinsage_hip import native as nv
    N = 300
    ins, exp = [], []
    for seed in (0, 1):
        t, g, rows = lb.epilogue_data(N, seed=seed)
        t = np.array(t)
        t[rows["nan_row"], N - 1] = 1.0
        ins.append({"t": _c(t), "g": _c(g)})
        exp.append({"gz": lb.epilogue_bwd_exact(t, g, True, True, lb.vec_of(N))})
    M = ins[0]["t"].shape[0]
    return Case(name, [I("t"), I("g"), M, N, nv.PS_RELU | nv.PS_L2NORM, O("gz"), ST], tuple(ins), {"gz": ((M, N), np.float32)}, tuple(exp))
