"""tests/helpers/bn_bwd_cases.py on the CPU: the exact restatement of ps_bn_bwd against its float64 closed form within the bound the
helper's docstring derives, the closed form (and through it the restatement) against torch float64 autograd of
F.normalize(F.relu(F.batch_norm(z, training=True))), the launcher's gates, the variants and the data condition.

The restatement takes mean / var / scale as fp32 inputs (the kernel does); autograd differentiates through the exact statistics.
So the comparison with autograd goes over the closed form: |restatement - autograd| <= bound(restatement, closed form at the fp32
statistics) + |closed form at the fp32 statistics - closed form at the exact statistics| + |closed form at the exact statistics -
autograd|, the middle term computed in float64 from the two sets of inputs and the last held to 1e-9 of the gradient's scale."""
import numpy as np
import pytest

from helpers import bn_bwd_cases as bb

SMALL = [n for n in bb.NAMES if n != "finish-unroll"]       # 4229 rows: the bound test alone runs it, with both flags


def _args(d):
    return d["z"], d["gy"], d["mean"], d["var"], d["scale"], d["beta"], bb.EPS


def _plain_rows(d):
    return np.array([r for r in range(d["M"]) if r not in bb.planted_rows(d)], dtype=np.int64)


@pytest.mark.parametrize("name", bb.NAMES)
def test_every_case_names_gates_it_reaches(name):
    _, M, N, off, gates = bb.case(name)
    assert gates
    f = bb.facts(M, N, off)
    for g in gates:
        assert bb.GATES[g](f), (name, g, f)


def test_every_gate_is_reached():
    reached = set()
    for _, M, N, off, _ in bb.CASES:
        f = bb.facts(M, N, off)
        reached |= {g for g, pred in bb.GATES.items() if pred(f)}
    assert reached == set(bb.GATES), sorted(set(bb.GATES) - reached)
    named = {g for c in bb.CASES for g in c[4]}
    assert named == set(bb.GATES), sorted(set(bb.GATES) - named)


def test_workspace_formula_is_the_librarys():
    from pinsage_hip import native as nv
    fn = nv.lib().ps_bn_bwd_workspace_bytes
    for _, M, N, off, _ in bb.CASES:
        assert fn(M, N) == bb.facts(M, N, off)["workspace_bytes"]
    assert fn(1, 8) == 0 and fn(2, 0) == 0


@pytest.mark.parametrize("plants", [False, True])
@pytest.mark.parametrize("name", bb.NAMES)
def test_data_condition(name, plants):
    """every float64 pre-activation outside the planted rows is at least MIN_PRE from zero; the planted rows are as planted"""
    d = bb.data(name, plants)
    a = bb.pre64(d["z"], d["mean"], d["scale"], d["beta"])
    rows = _plain_rows(d)
    assert np.abs(a[rows]).min() >= bb.MIN_PRE
    assert d["var"][d["N"] - 1] == 0 or d["N"] == 1
    if d["neg_row"] is not None:
        assert (a[d["neg_row"]] < 0).all() and not d["gy"][d["gy0_row"]].any()
        for row, v in ((d["above_row"], 2.0 ** -39), (d["below_row"], 2.0 ** -41)):
            rest = np.delete(a[row], d["clamp_col"])
            assert (rest < 0).all() and abs(a[row, d["clamp_col"]] / v - 1) < 1e-6
        assert d["scale"][d["gamma0_col"]] == 0 and d["beta"][d["gamma0_col"]] < 0
    if not plants:
        mean, var, _ = bb.exact_stats_64(d["z"], d["gamma"], bb.EPS)
        assert (mean.astype(np.float32) == d["mean"]).all() and (var.astype(np.float32) == d["var"]).all()


def test_restatement_within_its_bound_34_partitions():
    test_restatement_within_its_bound("finish-unroll", True, True)


@pytest.mark.parametrize("relu,l2", bb.FLAGSETS)
@pytest.mark.parametrize("name", SMALL)
def test_restatement_within_its_bound(name, relu, l2):
    d = bb.data(name, False)
    vec = bb.facts(d["M"], d["N"], bb.case(name)[3])["vec"]
    got = bb.bn_bwd_exact(*_args(d), relu, l2, vec)
    ref = bb.bn_bwd_64(*_args(d), relu, l2)
    bound = bb.bn_bwd_bound(*_args(d), relu, l2, vec)
    assert bound["et"].max() < 0.01 * bb.MIN_PRE                       # the ReLU masks the same elements in fp32 and float64
    for k in ("gz", "dgamma", "dbeta"):
        assert got[k].dtype == np.float32 and np.isfinite(got[k]).all()
        assert bb.outside(got[k], ref[k], bound[k]) == [], k


@pytest.mark.parametrize("relu,l2", bb.FLAGSETS)
@pytest.mark.parametrize("name", ["p129", "ragged-steps", "vec1-2blocks", "vec4-2blocks", "v4-keep+1"])
def test_restatement_against_autograd(name, relu, l2):
    d = bb.data(name, False)
    vec = bb.facts(d["M"], d["N"], bb.case(name)[3])["vec"]
    got = bb.bn_bwd_exact(*_args(d), relu, l2, vec)
    at32 = bb.bn_bwd_64(*_args(d), relu, l2)
    bound = bb.bn_bwd_bound(*_args(d), relu, l2, vec)
    mean, var, scale = bb.exact_stats_64(d["z"], d["gamma"], bb.EPS)
    at64 = bb.bn_bwd_64(d["z"], d["gy"], mean, var, scale, d["beta"], bb.EPS, relu, l2)
    auto = bb.autograd_64(d["z"], d["gy"], d["gamma"], d["beta"], bb.EPS, relu, l2)
    assert np.abs(at64["a"]).min() >= 0.5 * bb.MIN_PRE
    for k in ("gz", "dgamma", "dbeta"):
        # the constant column: autograd's gradient of gamma there is that of rstd = 1 / sqrt(eps) times an exact zero, as here
        scale_k = max(np.abs(auto[k]).max(), 1e-30)
        assert np.abs(at64[k] - auto[k]).max() <= 1e-9 * scale_k, k
        slack = np.abs(at32[k] - at64[k]) + 1e-9 * scale_k
        assert bb.outside(got[k], auto[k], bound[k] + slack) == [], k


@pytest.mark.parametrize("variant", bb.VARIANTS)
def test_every_variant_is_detected(variant):
    """each wrong order of operations differs from the restatement in some output of some case: the bit-for-bit tests have power"""
    hit = []
    for name in ("ragged-steps", "vec4-2blocks", "p129"):
        d = bb.data(name, True)
        vec = bb.facts(d["M"], d["N"], bb.case(name)[3])["vec"]
        for relu, l2 in bb.FLAGSETS:
            want = bb.expected(name, relu, l2)
            got = bb.bn_bwd_exact(*_args(d), relu, l2, vec, variant=variant, gamma=d["gamma"])
            hit += [k for k in want if want[k].tobytes() != got[k].tobytes()]
    assert hit, variant


def test_planted_rows_and_columns():
    """under ReLU + norm: the all-negative row adds nothing to the column sums and its gz is the column term alone; the gamma = 0
    column's gz is zero; the row with gy = 0 has ga = 0"""
    d = bb.data("vec4-2blocks", True)
    e = bb.expected("vec4-2blocks", True, True)
    g0 = d["gamma0_col"]
    assert not e["gz"][:, g0].any() and e["dgamma"][g0] == 0 and e["dbeta"][g0] == 0
    z2 = np.array(d["z"])
    z2[d["neg_row"]] -= 1.0                                        # still masked: the sums do not move
    e2 = bb.bn_bwd_exact(z2, d["gy"], d["mean"], d["var"], d["scale"], d["beta"], bb.EPS, True, True, 4)
    assert e2["dgamma"].tobytes() == e["dgamma"].tobytes() and e2["dbeta"].tobytes() == e["dbeta"].tobytes()
    gy2 = np.array(d["gy"])
    gy2[d["neg_row"]] *= 2.0                                       # nor with its gy
    e3 = bb.bn_bwd_exact(d["z"], gy2, d["mean"], d["var"], d["scale"], d["beta"], bb.EPS, True, True, 4)
    assert e3["gz"].tobytes() == e["gz"].tobytes()
    assert np.isfinite(e["gz"]).all()
