"""The cases of the contract matrix (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py) for the layer norm, csrc/layer_norm.hip:
ps_layer_norm and ps_layer_norm_bwd.  Every output is held to ln_cases' numpy restatement bit for bit (no eager expectation).

The builders are written exactly as abi_cases' own and join its CASES table through its `case` decorator when this module is
imported; tests/test_abi_a_layer_norm_case.py imports it, and is collected before the test modules that read the table;
tests/test_hip_layer_norm.py imports it too and starts the contract matrix for the two entry points itself."""
import functools

import numpy as np

from helpers import abi_cases as ac
from helpers.abi_cases import I, O, WS, WSB, ST, Case, _c

M, N = 131, 300


@functools.lru_cache(maxsize=None)
def _sets():
    """two input sets and their restated outputs: M = 131 (two partitions, the second of three rows), N = 300 (16-byte sweeps, two
    sweeps, two column blocks), dead rows at the head, inside the first partition and in the second; no NaN"""
    from helpers import ln_cases as ln
    f = ln.facts(M, N)
    assert f["P"] == 2 and f["vec"] == 4 and f["col_blocks"] == 2 and f["sweeps"] == 2 and f["workspace_bytes"] > 0
    out = []
    for seed in (1, 2):
        rs = np.random.RandomState(9900 + seed)
        x = (0.3 + 1.5 * rs.standard_normal((M, N))).astype(np.float32)
        gy = rs.standard_normal((M, N)).astype(np.float32)
        gamma = rs.uniform(0.5, 1.5, N).astype(np.float32)
        beta = (0.5 * rs.standard_normal(N)).astype(np.float32)
        live = np.ones(M, dtype=np.int32)
        live[[0, 17 + seed, 127, 129]] = (0, -1, 0, 0)
        fwd = ln.ln_fwd_exact(x, gamma, beta, ln.EPS, live, f["vec"])
        bwd = ln.ln_bwd_exact(x, gy, fwd["mean"], fwd["rstd"], gamma, live, f["vec"])
        assert all(np.isfinite(v).all() for v in list(fwd.values()) + list(bwd.values()))
        out.append((dict(x=_c(x), gy=_c(gy), gamma=_c(gamma), beta=_c(beta), live=_c(live)), fwd, bwd))
    return tuple(out)


@ac.case
def _ps_layer_norm(name):
    from helpers import ln_cases as ln
    sets = _sets()
    ins = tuple({k: s[0][k] for k in ("x", "gamma", "beta", "live")} for s in sets)
    return Case(name, [I("x"), M, N, I("gamma"), I("beta"), float(ln.EPS), I("live"), O("y"), O("mean"), O("rstd"), ST], ins,
                {"y": ((M, N), np.float32), "mean": ((M,), np.float32), "rstd": ((M,), np.float32)}, tuple(s[1] for s in sets))


@ac.case
def _ps_layer_norm_bwd(name):
    sets = _sets()
    ins = tuple(dict(x=s[0]["x"], gy=s[0]["gy"], mean=s[1]["mean"], rstd=s[1]["rstd"], gamma=s[0]["gamma"], live=s[0]["live"])
                for s in sets)
    return Case(name, [I("x"), I("gy"), M, N, I("mean"), I("rstd"), I("gamma"), I("live"), O("gx"), O("dgamma"), O("dbeta"), WS, WSB,
                       ST], ins,
                {"gx": ((M, N), np.float32), "dgamma": ((N,), np.float32), "dbeta": ((N,), np.float32)}, tuple(s[2] for s in sets),
                ws=("ps_layer_norm_bwd_workspace_bytes", (M, N)))
