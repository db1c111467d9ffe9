"""The batch-norm cases of tests/helpers/bn_cases.py without a GPU: the tables are the ones the kernels' gates ask for and reach
every gate that tests/helpers/layers_cases.py's tables leave out (by the same restated launcher), every statistics column is
decided, the exact restatements lie inside the bounds the fp64 references are held to in tests/test_hip_layers.py, and the cases
tell the restatements from five near misses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bn_cases as bc  # noqa: E402
import layers_cases as lc  # noqa: E402

U = 2.0 ** -53
SMALL_STATS = [n for n in bc.STATS_NAMES if bc.stats_case(n)[1] <= 1 << 20]


def test_tables_are_the_issues():
    assert len(set(bc.STATS_NAMES)) == len(bc.STATS_CASES) and len(set(bc.APPLY_NAMES)) == len(bc.APPLY_CASES)
    assert [c[1:4] for c in bc.STATS_CASES] == [(2, 1, 0), (127, 4, 0), (128, 4, 0), (129, 4, 0), (161, 8, 0), (129, 65, 0),
                                                (37, 260, 0), (129, 256, 1), (4229, 8, 0), (8388609, 4, 0)]
    assert [c[1:5] for c in bc.APPLY_CASES] == [(1, 1, 0, 0), (5, 1024, 0, 0), (5, 1028, 0, 0), (3, 2052, 0, 0), (5, 256, 1, 0),
                                                (5, 257, 0, 0), (3, 515, 0, 0), (16389, 8, 0, 0), (9, 1028, 0, 1)]
    assert (bc.BN_ROWS, bc.EPS, bc.MOMENTUM) == (lc.S, lc.EPS, lc.MOMENTUM)
    assert all(c[-1] for c in bc.STATS_CASES + bc.APPLY_CASES)                  # every row names its gate


def test_rows_reach_the_gates_they_name():
    f = {c[0]: bc.facts(c) for c in bc.STATS_CASES}
    assert f["min"]["vec"] == 1 and f["min"]["P"] == 1
    assert [f[n]["P"] for n in ("p127", "p128", "p129")] == [1, 1, 2] and f["p129"]["last_rows"] == 1 and f["p129"]["vec"] == 4
    assert f["ragged-steps"]["last_rows"] == 33 and (2, 1, 1, 1) in f["ragged-steps"]["wave_steps"]
    assert f["vec1-2blocks"]["vec"] == 1 and f["vec1-2blocks"]["col_blocks"] == 2 and 65 - 64 == 1
    assert f["vec4-2blocks"]["vec"] == 4 and f["vec4-2blocks"]["col_blocks"] == 2 and 260 - 256 == 4
    assert f["vec1-offset"]["vec"] == 1 and f["vec1-offset"]["col_blocks"] == 4
    assert f["finish-unroll"]["P"] == 34 and (f["finish-unroll"]["finish_unrolled"], f["finish-unroll"]["finish_rest"]) == (1, 2)
    assert f["partial-second-pass"]["P"] == 65537 and f["partial-second-pass"]["grid"][0] == 65535 and f["partial-second-pass"]["passes"] == 2
    assert f["partial-second-pass"]["workspace_bytes"] == 65537 * 2 * 4 * 8
    a = {c[0]: bc.facts(c) for c in bc.APPLY_CASES}
    assert [(a[n]["vec"], a[n]["sweeps"], a[n]["fits"], a[n]["beyond"]) for n in ("v4-keep", "v4-keep+1", "v4-long")] == \
        [(4, 4, True, 0), (4, 5, False, 1), (4, 9, False, 5)]
    assert a["v4-keep+1"]["tail_cols"] == 4
    assert [(a[n]["vec"], a[n]["sweeps"], a[n]["fits"], a[n]["beyond"]) for n in ("v1-keep", "v1-keep+1", "v1-long")] == \
        [(1, 4, True, 0), (1, 5, False, 1), (1, 9, False, 5)]
    assert a["v1-keep+1"]["tail_cols"] == 1
    assert a["rows-second-pass"]["passes"] == 2 and a["rows-second-pass"]["grid"] == 4096
    assert (a["v1-by-beta"]["vec"], a["v1-by-beta"]["sweeps"]) == (1, 17) and bc.apply_facts(9, 1028)["vec"] == 4
    assert a["min"] == dict(kernel="apply", vec=1, sweeps=1, fits=True, beyond=0, tail_cols=1, grid=1, passes=1)


def test_new_rows_reach_what_the_old_tables_do_not():
    """the gates of bc.GATES: no (shape, offset) that tests/test_hip_layers.py runs reaches one, a row of the new tables does"""
    old_shapes = [(M, N, 0) for M in lc.STATS_M for N in lc.STATS_N] + [lc.OFFSET_SHAPE + (1,)]
    old = [bc.stats_facts(M, N, o) for M, N, o in old_shapes] + [bc.apply_facts(M, N, o, o) for M, N, o in old_shapes]
    old.append(bc.apply_facts(16384, 256))                                       # test_graph_conv_layer_peak_memory's layer
    new = {"stats " + c[0]: bc.facts(c) for c in bc.STATS_CASES}
    new.update({"apply " + c[0]: bc.facts(c) for c in bc.APPLY_CASES})
    for gate, reached in bc.GATES.items():
        assert not any(reached(f) for f in old), gate
        rows = [n for n, f in new.items() if reached(f)]
        print(f"{gate}: {rows}")
        assert rows, gate
    # what the old tables do reach of the long-row path: one sweep beyond KEEP, scalar, four columns
    assert max(f["beyond"] for f in old if f["kernel"] == "apply") == 1
    assert max(f["passes"] for f in old) == 1 and max(f["P"] for f in old if f["kernel"] == "stats") == 71


@pytest.mark.parametrize("name", bc.STATS_NAMES)
def test_every_statistics_column_is_decided(name):
    d, e = bc.stats_data(name), bc.stats_expected(name)
    assert e["part"].shape == (bc.facts(bc.stats_case(name))["P"], 2, d["N"]) and e["part"].dtype == np.float64
    for k in bc.OUTPUTS:
        assert e[k].dtype == np.float32 and e[k].shape == (d["N"],)
        assert e["decided"][k].all(), (k, np.nonzero(~e["decided"][k])[0])
    if d["N"] >= 2:                                           # the constant column: exact sums, mean CONST, variance +0.0
        assert e["mean"][-1] == bc.CONST and e["var"][-1] == 0 and not np.signbit(e["var"][-1])
        assert e["part"][0, 0, -1] == min(d["M"], bc.BN_ROWS) * float(bc.CONST)
    if d["M"] >= 3:                                           # the planted column is what it claims to be
        z0 = d["z"][:, 0].astype(np.float64)
        assert (z0 * z0).mean() / z0.var() > 1e5


def test_an_undecided_column_is_reported():
    """layers_cases' constant 3.7f: its variance is a cancellation residue that the quotient's last bit decides"""
    rs = np.random.RandomState(1)
    z = rs.standard_normal((127, 4)).astype(np.float32)
    z[:, 3] = np.float32(3.7)
    e = bc.stats_exact(z, np.ones(4, dtype=np.float32), np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.float32))
    assert not e["decided"]["var"][3] and e["decided"]["mean"][3] and e["decided"]["var"][:3].all()


@pytest.mark.parametrize("name", bc.STATS_NAMES)
def test_statistics_restatement_is_inside_the_fp64_bounds(name):
    """tests/test_hip_layers.py::test_bn_batch_stats' bounds around layers_cases.bn_stats_ref"""
    d, e = bc.stats_data(name), bc.stats_expected(name)
    M = d["M"]
    ref = lc.bn_stats_ref(d["z"], d["gamma"], d["rm0"], d["rv0"])
    mean_tol = (2.0 ** -23 + 2 * M * U) * np.abs(ref["mean"])
    var_tol = 2.0 ** -23 * ref["var"] + 2 * M * U * ref["ez2"]
    scale_tol = np.abs(ref["scale"]) * (2.0 ** -23 + 0.5 * var_tol / (ref["var"] + lc.EPS))
    m = lc.MOMENTUM
    rm_tol = m * mean_tol + 2.0 ** -22 * ((1 - m) * np.abs(d["rm0"]) + m * np.abs(ref["mean"]))
    rv_tol = m * var_tol * M / (M - 1) + 2.0 ** -22 * ((1 - m) * np.abs(d["rv0"]) + m * ref["var"] * M / (M - 1))
    for k, tol in (("mean", mean_tol), ("var", var_tol), ("scale", scale_tol), ("rm", rm_tol), ("rv", rv_tol)):
        err = np.abs(e[k].astype(np.float64) - ref[k])
        assert (err <= tol).all(), (k, int(np.argmax(err - tol)), float(np.max(err - tol)))


@pytest.mark.parametrize("name", bc.APPLY_NAMES)
def test_apply_restatement_is_inside_the_fp64_tolerance(name):
    """tests/test_hip_layers.py::test_bn_apply's rtol / atol around layers_cases.bn_apply_ref; the planted rows are what they say"""
    d = bc.apply_data(name)
    vec = bc.facts(bc.apply_case(name))["vec"]
    for relu in (False, True):
        for l2 in (False, True):
            got = bc.apply_exact(d["z"], d["mean"], d["scale"], d["beta"], relu, l2, vec)
            with np.errstate(invalid="ignore"):
                ref = lc.bn_apply_ref(d["z"], d["mean"], d["scale"], d["beta"], relu, l2)
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, ref, rtol=lc.RTOL, atol=lc.ATOL)                  # NaNs in the same places
            if d["neg_row"] is None:
                continue
            row = got[d["neg_row"]]
            if relu:
                assert not row.any() and not np.signbit(row).any()                            # +0.0, through the 1e-12 clamp too
            else:
                assert (row < 0).all()
            nan = np.isnan(got)
            if l2:
                assert nan[d["nan_row"]].all() and nan.sum() == d["N"]                         # the whole row, and no other
            else:
                assert nan[d["nan_row"], -1] and nan.sum() == 1


@pytest.mark.parametrize("variant", bc.VARIANTS_STATS)
def test_cases_tell_the_statistics_from_a_near_miss(variant):
    differing = []
    for name in SMALL_STATS:
        d, e = bc.stats_data(name), bc.stats_expected(name)
        v = bc.stats_exact(d["z"], d["gamma"], d["rm0"], d["rv0"], variant=variant)
        parts = v["part"].shape != e["part"].shape or not np.array_equal(v["part"], e["part"])
        outs = [k for k in bc.OUTPUTS if not np.array_equal(v[k], e[k])]
        if parts or outs:
            differing.append((name, "workspace" if parts else "", outs))
    print(variant, "differs on", differing)
    assert differing
    assert any(w for _, w, _ in differing)                    # the workspace comparison sees every one of them


@pytest.mark.parametrize("variant", bc.VARIANTS_APPLY)
def test_cases_tell_the_l2_sum_from_a_near_miss(variant):
    differing = []
    for name in bc.APPLY_NAMES:
        if name == "rows-second-pass":                             # eight columns: covered by the wide rows
            continue
        d = bc.apply_data(name)
        vec = bc.facts(bc.apply_case(name))["vec"]
        want = bc.apply_exact(d["z"], d["mean"], d["scale"], d["beta"], True, True, vec)
        got = bc.apply_exact(d["z"], d["mean"], d["scale"], d["beta"], True, True, vec, variant=variant)
        if bc.mismatches(got, want):
            differing.append(name)
    print(variant, "differs on", differing)
    assert differing


def test_wave_sum_is_the_dpp_sequence():
    """bc.wave_sum (a balanced tree) against ps_wave_sum_f32's six DPP steps emulated lane by lane (csrc/ps_common.h): quad_perm
    [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3 (a lane
    a step does not reach adds 0), lane 63 read"""
    rs = np.random.RandomState(5)
    v = (rs.standard_normal((50, 64)) * 1000.0 ** rs.uniform(-1, 1, size=(50, 64))).astype(np.float32)
    want = bc.wave_sum(v)
    lane = np.arange(64)
    zero = np.zeros((50, 64), dtype=np.float32)
    v = v + v[:, lane ^ 1]
    v = v + v[:, lane ^ 2]
    v = v + v[:, (lane & ~7) | (7 - (lane & 7))]
    v = v + v[:, (lane & ~15) | (15 - (lane & 15))]
    v = v + np.where((lane // 16) % 2 == 1, v[:, np.maximum(lane // 16 * 16 - 1, 0)], zero)
    v = v + np.where(lane >= 32, v[:, np.full(64, 31)], zero)
    assert np.array_equal(v[:, 63], want)
    assert not np.array_equal(want, np.cumsum(v, axis=1, dtype=np.float32)[:, -1])
