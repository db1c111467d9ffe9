"""The restatement of ps_spmm_csr_exact / ps_sddmm_csr (tests/helpers/spmm_cases.py) is itself checked here, without a GPU:
against float64 closed forms within the bounds derived there, against torch CPU autograd (float64) of the index_add_ formulation
within the same bounds, and the case table against what it says it plants."""
import numpy as np
import pytest
import torch

from helpers import spmm_cases as sc

NAMES = sc.names()


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} entries beyond the bound, worst {err[bad].max()} against {bound[bad].min()}"


def test_slice_length_comes_from_the_library():
    from pinsage_hip import native
    S = sc.slice_len()
    assert S == native.lib().ps_spmm_exact_slice() and S >= 64 and S % 64 == 0
    assert native.lib().ps_spmm_csr_exact_workspace_bytes(0, 8) == 0
    assert native.lib().ps_spmm_csr_exact_workspace_bytes(4 * S, 8) >= 2 * 4 * 8 * 4


def test_case_table_plants_what_it_says():
    S = sc.slice_len()
    seen = set()
    for name in NAMES:
        c = sc.case(name)
        pc = sc.pieces(c["rowptr"], S)
        for r, want in c["want"].items():
            assert pc[r] == want, (name, r, pc[r], want)
        assert c["E"] <= 4 * S + 64 and c["rowptr"][-1] == c["E"] == len(c["col"])
        assert np.array_equal(c["s_col"], c["rows"][c["index"]]) and np.array_equal(np.sort(c["index"]), np.arange(c["E"]))
        assert (np.diff(c["col"][c["index"]]) >= 0).all() and c["s_rowptr"][-1] == c["E"]
        seen.add((c["vec"], c["val"] is None))
    c = sc.case("single")
    assert c["V"] == c["E"] == c["H"] == 1
    c = sc.case("short")
    deg = np.diff(c["rowptr"])
    assert c["E"] < S and c["H"] == 4 and (deg == 0).sum() >= 5 and (deg > 0).sum() >= 10 and ((deg[:-1] == 0) & (deg[1:] > 0)).any()
    c = sc.case("straddle")
    assert (c["rowptr"][1], c["rowptr"][2]) == (S - 3, S + 5)
    c = sc.case("abut")
    assert c["rowptr"][2] == S and all(len(p) <= 1 for p in sc.pieces(c["rowptr"], S))
    c = sc.case("one-slice")
    assert (c["rowptr"][0], c["rowptr"][1], c["rowptr"][2]) == (0, S, 2 * S)
    c = sc.case("two-slices")
    assert (c["rowptr"][0], c["rowptr"][1]) == (0, 2 * S)
    c = sc.case("hub")
    assert (c["rowptr"][1], c["rowptr"][2]) == (S - 1, 3 * S + 1)
    c = sc.case("meet")
    assert S < c["rowptr"][2] < 2 * S and c["rowptr"][1] < S and c["rowptr"][3] > 2 * S
    c = sc.case("empties")
    deg = np.diff(c["rowptr"])
    assert not deg[:3].any() and not deg[-2:].any() and c["E"] % S and c["val"] is None
    assert sc.case("scalar")["H"] == 10 and sc.case("scalar")["vec"] == 1
    c = sc.case("two-sweeps")
    assert c["H"] == 300 and c["vec"] == 4 and 256 < c["H"] < 512
    c = sc.case("offset")
    assert c["H"] == 8 and c["offset"] == 1 and c["vec"] == 1
    assert sc.case("no-val")["val"] is None and sc.case("no-val")["plants"]
    c = sc.case("outside")
    assert c["N"] < c["V"] and (c["col"] >= c["N"]).sum() > 10 and (c["col"] < c["N"]).sum() > 10
    assert seen == {(1, False), (4, False), (4, True)}


@pytest.mark.parametrize("name", [n for n in NAMES if sc.case(n)["plants"] and sc.case(n)["H"] <= 10])
def test_planted_triples_pin_the_slices_and_the_order(name):
    """Every element of a cut row holds a 1 that survives only because a piece ends between 2^24 + 2^22 and it: the restatement with
    another slice length, or as one chain, differs from the restatement with S in EVERY column of every planted row."""
    c = sc.case(name)
    S = c["S"]
    want = sc.expected(name)["out"]
    rows = sorted({r for r, _ in c["plants"]})
    assert rows == [r for r, p in enumerate(sc.pieces(c["rowptr"], S)) if len(p) > 1]
    assert (want[rows] % 2 == 1).all()                            # the 1 is kept in every column
    for b_row, b in c["plants"]:
        assert list(c["col"][b - 1:b + 2]) == [0, 1, 2] and b % S == 0
        assert c["val"] is None or list(c["val"][b - 1:b + 2]) == [1.0, 1.0, 1.0]
    assert (c["x"][0] == 2.0 ** 24 + 2.0 ** 22).all() and (c["x"][1] == 1).all() and (c["x"][2] == -3 * 2.0 ** 22).all()
    for other in (S - 1, S + 1, 2 * S, 1 << 40):
        got = sc.spmm_exact(c["rowptr"], c["col"], c["val"], c["x"], other)
        moved = [r for r, b in c["plants"] if b % other]           # slices of 2 S keep the boundaries at even multiples of S
        assert moved and (got[moved] != want[moved]).all(), (name, other)
        rest = np.setdiff1d(np.arange(c["V"]), rows)
        if other == 1 << 40:                                      # rows inside one slice do not depend on S
            assert np.array_equal(got[rest].view(np.uint32), want[rest].view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_float64(name):
    c = sc.case(name)
    e = sc.expected(name)
    out64, bound = sc.spmm_64(c["rowptr"], c["col"], c["val"], c["x"], c["S"])
    _within(e["out"], out64, bound, f"{name} out")
    dx64, bound = sc.spmm_64(c["s_rowptr"], c["s_col"], c["s_val"], c["g"], c["S"])
    _within(e["dx"], dx64, bound, f"{name} dx")
    d64, bound = sc.sddmm_64(c["rowptr"], c["col"], c["x"], c["g"], c["vec"])
    _within(e["dval"], d64, bound, f"{name} dval")
    empty = np.diff(c["rowptr"]) == 0
    assert not e["out"][empty].view(np.uint32).any()             # +0.0, not -0.0
    skipped = c["col"] >= c["N"]
    assert not e["dval"][skipped].view(np.uint32).any()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_torch_autograd(name):
    """out = zeros.index_add_(0, target, x[source] * val) in float64 on the CPU; its autograd gradients for g are what the
    restatement computes as dx (the SpMM over the source-grouped edges) and dval (the row dots), within the derived bounds"""
    c = sc.case(name)
    e = sc.expected(name)
    ok = c["col"] < c["N"]                                       # edges whose source the kernel skips take no part
    rows = torch.tensor(c["rows"][ok])
    cols = torch.tensor(c["col"][ok].astype(np.int64))
    x = torch.tensor(c["x"].astype(np.float64), requires_grad=True)
    val_h = np.ones(c["E"]) if c["val"] is None else c["val"].astype(np.float64)
    val = torch.tensor(val_h, requires_grad=True)
    out = torch.zeros((c["V"], c["H"]), dtype=torch.float64).index_add_(0, rows, x[cols] * val[torch.tensor(np.nonzero(ok)[0])][:, None])
    out.backward(torch.tensor(c["g"].astype(np.float64)))
    _, bound = sc.spmm_64(c["rowptr"], c["col"], c["val"], c["x"], c["S"])
    _within(e["out"], out.detach().numpy(), bound, f"{name} out")
    _, bound = sc.spmm_64(c["s_rowptr"], c["s_col"], c["s_val"], c["g"], c["S"])
    _within(e["dx"][:c["N"]], x.grad.numpy(), bound[:c["N"]], f"{name} dx")
    _, bound = sc.sddmm_64(c["rowptr"], c["col"], c["x"], c["g"], c["vec"])
    _within(e["dval"], val.grad.numpy(), bound, f"{name} dval")


def test_sweep_width_is_part_of_the_dot():
    """the 16-byte and the scalar sweep chain different columns per lane: the restatement must be told which one ran"""
    c = sc.case("two-sweeps")
    assert not np.array_equal(sc.sddmm_exact(c["rowptr"], c["col"], c["x"], c["g"], 1), sc.expected("two-sweeps")["dval"])
