"""The case of the contract matrix (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py) for the batch-norm layer's backward,
csrc/batch_norm_bwd.hip: ps_bn_bwd.  All three outputs are held to bn_bwd_cases' numpy restatement bit for bit (no eager
expectation).

The builder is written exactly as abi_cases' own and joins its CASES table through its `case` decorator when this module is
imported; tests/test_abi_bn_bwd_case.py imports it, and is collected before the test modules that read the table;
tests/test_hip_bn_bwd.py imports it too and starts the contract matrix for this entry point itself."""
import numpy as np

from helpers import abi_cases as ac
from helpers.abi_cases import I, O, WS, WSB, ST, Case, _c


@ac.case
def _ps_bn_bwd(name):
    """ReLU and row norm, M = 131 (two partitions, the second of three rows), N = 300: 16-byte sweeps, two column blocks, rows
    longer than one sweep; gz, dgamma and dbeta bit for bit; no NaN"""
    from helpers import bn_bwd_cases as bb
    from helpers import bn_cases as bc
    from pinsage_hip import native as nv
    M, N = 131, 300
    f = bb.facts(M, N)
    assert f["P"] == 2 and f["vec"] == 4 and f["col_blocks"] == 2 and f["workspace_bytes"] > 0
    ins, exp = [], []
    for seed in (1, 2):
        rs = np.random.RandomState(8800 + seed)
        z = (0.3 + 1.5 * rs.standard_normal((M, N))).astype(np.float32)
        z[:, 0] = (100.0 + 0.05 * rs.standard_normal(M)).astype(np.float32)
        z[:, N - 1] = bc.CONST
        gamma = rs.uniform(0.5, 1.5, N).astype(np.float32)
        beta = (0.5 * rs.standard_normal(N)).astype(np.float32)
        gy = rs.standard_normal((M, N)).astype(np.float32)
        mean, var, scale = bb._stats(z, gamma)
        s = {"z": _c(z), "gy": _c(gy), "mean": _c(mean), "var": _c(var), "scale": _c(scale), "beta": _c(beta)}
        e = bb.bn_bwd_exact(z, gy, mean, var, scale, beta, bb.EPS, True, True, f["vec"])
        assert all(np.isfinite(v).all() for v in e.values())
        ins.append(s)
        exp.append(e)
    return Case(name, [I("z"), I("gy"), M, N, I("mean"), I("var"), I("scale"), I("beta"), float(bb.EPS), nv.PS_RELU | nv.PS_L2NORM,
                       O("gz"), O("dgamma"), O("dbeta"), WS, WSB, ST], tuple(ins),
                {"gz": ((M, N), np.float32), "dgamma": ((N,), np.float32), "dbeta": ((N,), np.float32)}, tuple(exp),
                ws=("ps_bn_bwd_workspace_bytes", (M, N)))
