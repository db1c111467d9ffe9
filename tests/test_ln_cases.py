"""tests/helpers/ln_cases.py on the CPU: the exact restatements of ps_layer_norm and ps_layer_norm_bwd against their float64 closed
forms within the bounds the helper's docstring derives, the closed forms against torch float64 autograd of F.layer_norm followed by
the torch.where, the launcher's gates, the variants, the planted rows, and the python surface that needs no device: the three
prototypes and ImportanceAggregator's switch.

The backward's restatement takes mean / rstd as fp32 inputs (the kernel does): its closed form is evaluated at those.  Autograd
differentiates through the exact statistics, so the closed form is held to autograd at the float64 mean and rstd."""
import numpy as np
import pytest
import torch

from helpers import ln_cases as ln

SMALL = [n for n in ln.NAMES if n != "finish-unroll"]       # 4229 rows: one mask only
FWD, BWD = ("y", "mean", "rstd"), ("gx", "dgamma", "dbeta")


@pytest.mark.parametrize("name", ln.NAMES)
def test_every_case_names_gates_it_reaches(name):
    _, M, N, off, gates = ln.case(name)
    assert gates
    f = ln.facts(M, N, off)
    for g in gates:
        assert ln.GATES[g](f), (name, g, f)


def test_every_gate_is_reached():
    named = {g for c in ln.CASES for g in c[4]}
    assert named == set(ln.GATES), sorted(set(ln.GATES) - named)


def test_workspace_formula_is_the_librarys():
    from pinsage_hip import native as nv
    fn = nv.lib().ps_layer_norm_bwd_workspace_bytes
    for _, M, N, off, _ in ln.CASES:
        assert fn(M, N) == ln.facts(M, N, off)["workspace_bytes"] > 0
    assert fn(0, 8) == 0 and fn(2, 0) == 0


def test_the_masks_are_what_they_say():
    M = 161
    assert ln.mask("none", M) is None
    alive = {w: ln.alive_rows(ln.mask(w, M), M) for w in ln.MASKS}
    assert alive["none"].all() and not alive["all dead"].any()
    assert not alive["first row dead"][0] and alive["first row dead"][1:].all()
    assert not alive["last row of a partition dead"][127] and alive["last row of a partition dead"].sum() == M - 1
    assert not alive["a wholly dead partition"][:128].any() and alive["a wholly dead partition"][128:].all()
    assert {int(v) for v in ln.mask("a wholly dead partition", M)} == {-1, 0, 1, 7}


def _check(name, which):
    d = ln.data(name, False)
    vec = ln.facts(d["M"], d["N"], ln.case(name)[3])["vec"]
    live = ln.mask(which, d["M"])
    alive = ln.alive_rows(live, d["M"])
    x, gy = ln.poison(d["x"], live), ln.poison(d["gy"], live)          # the dead rows hold NaN and Inf
    got = ln.ln_fwd_exact(x, d["gamma"], d["beta"], ln.EPS, live, vec)
    ref = ln.ln_fwd_64(x, d["gamma"], d["beta"], ln.EPS, live)
    bound = ln.ln_fwd_bound(x, d["gamma"], d["beta"], ln.EPS, live, vec)
    for k in FWD:
        assert got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
        assert ln.outside(got[k], ref[k], bound[k]) == [], (name, which, k)
        assert not got[k][~alive].any() and not np.signbit(got[k][~alive]).any()
    bgot = ln.ln_bwd_exact(x, gy, got["mean"], got["rstd"], d["gamma"], live, vec)
    bref = ln.ln_bwd_64(x, gy, got["mean"], got["rstd"], d["gamma"], live)
    bbound = ln.ln_bwd_bound(x, gy, got["mean"], got["rstd"], d["gamma"], live, vec)
    for k in BWD:
        assert bgot[k].dtype == np.float32 and np.isfinite(bgot[k]).all(), k
        assert ln.outside(bgot[k], bref[k], bbound[k]) == [], (name, which, k)
    assert not bgot["gx"][~alive].any() and not np.signbit(bgot["gx"][~alive]).any()


@pytest.mark.parametrize("which", ln.MASKS)
@pytest.mark.parametrize("name", SMALL)
def test_restatement_within_its_bound(name, which):
    _check(name, which)


def test_restatement_within_its_bound_34_partitions():
    _check("finish-unroll", "a wholly dead partition")


@pytest.mark.parametrize("which", ln.MASKS)
@pytest.mark.parametrize("name", ["vec1-partial", "p129", "ragged-steps", "vec1-2blocks", "vec4-2blocks", "v4-keep+1"])
def test_closed_form_is_autograd(name, which):
    d = ln.data(name, False)
    live = ln.mask(which, d["M"])
    auto = ln.autograd_64(d["x"], d["gy"], d["gamma"], d["beta"], ln.EPS, live)
    f = ln.ln_fwd_64(d["x"], d["gamma"], d["beta"], ln.EPS, live)
    b = ln.ln_bwd_64(d["x"], d["gy"], f["mean"], f["rstd"], d["gamma"], live)
    for k, got in (("y", f["y"]), ("gx", b["gx"]), ("dgamma", b["dgamma"]), ("dbeta", b["dbeta"])):
        scale = max(np.abs(auto[k]).max(), 1e-30)
        assert np.abs(got - auto[k]).max() <= 1e-9 * scale, (name, which, k)


@pytest.mark.parametrize("variant", ln.VARIANTS)
def test_every_variant_is_detected(variant):
    """each wrong order of operations differs from the restatement in some output of some case: the bit-for-bit tests have power"""
    hit = []
    for name in ("ragged-steps", "vec4-2blocks", "p129", "vec1-offset"):
        d = ln.data(name, True)
        vec = ln.facts(d["M"], d["N"], ln.case(name)[3])["vec"]
        want = ln.expected(name)
        got = ln.ln_fwd_exact(d["x"], d["gamma"], d["beta"], ln.EPS, None, vec, variant=variant)
        got.update(ln.ln_bwd_exact(d["x"], d["gy"], want["mean"], want["rstd"], d["gamma"], None, vec, variant=variant))
        hit += [(name, k) for k in want if want[k].tobytes() != got[k].tobytes()]
    assert hit, variant


def test_planted_rows():
    """the constant row (var == 0, y = beta, rstd = 1 / sqrtf(eps)), the row of 100 +- 0.05 (the two-pass variance keeps it, the
    single-pass one does not), the row of zeros, and one NaN: its row is NaN, every dgamma is NaN, dbeta is finite, the other rows
    keep their bits"""
    name = "vec4-2blocks"
    d, e = ln.data(name), ln.expected(name)
    c, h, z = d["const_row"], d["hundred_row"], d["zero_row"]
    assert e["mean"][c] == ln.CONST and e["rstd"][c] == np.float32(1.0) / np.sqrt(np.float32(ln.EPS))
    assert e["y"][c].tobytes() == d["beta"].tobytes()
    assert e["mean"][z] == 0 and e["y"][z].tobytes() == d["beta"].tobytes()
    ref = ln.ln_fwd_64(d["x"], d["gamma"], d["beta"], ln.EPS, None)
    assert abs(e["rstd"][h] / ref["rstd"][h] - 1) < 1e-4                              # sigma = 0.05 survives two passes
    one = ln.ln_fwd_exact(d["x"], d["gamma"], d["beta"], ln.EPS, None, 4, variant=ln.VARIANTS[2])
    assert not abs(one["rstd"][h] / ref["rstd"][h] - 1) < 1e-2                        # and not E[x^2] - mean^2
    n = ln.expected(name, nan=True)
    r = d["nan_row"]
    assert np.isnan(n["y"][r]).all() and np.isnan(n["gx"][r]).all() and np.isnan(n["mean"][r]) and np.isnan(n["rstd"][r])
    assert np.isnan(n["dgamma"]).all() and np.isfinite(n["dbeta"]).all() and n["dbeta"].tobytes() == e["dbeta"].tobytes()
    rest = np.arange(d["M"]) != r
    for k in ("y", "gx", "mean", "rstd"):
        assert n[k][rest].tobytes() == e[k][rest].tobytes() and np.isfinite(n[k][rest]).all(), k


# ---- the python surface that needs no device ---------------------------------------------------------------------------------------
def test_the_three_symbols_have_prototypes():
    from pinsage_hip import native as nv
    assert nv.PROTOTYPES["ps_layer_norm"] == "i pqippfppppp"
    assert nv.PROTOTYPES["ps_layer_norm_bwd_workspace_bytes"] == "z qi"
    assert nv.PROTOTYPES["ps_layer_norm_bwd"] == "i ppqippppppppzp"
    assert all(hasattr(nv.lib(), n) for n in ("ps_layer_norm", "ps_layer_norm_bwd_workspace_bytes", "ps_layer_norm_bwd"))


def test_norm_method_defaults_to_torch_and_rejects_other_values():
    from model.aggregators import ImportanceAggregator
    assert ImportanceAggregator.norm_method == "torch"
    m = ImportanceAggregator(6, 4)
    assert m.norm_method == "torch"
    m.norm_method = "triton"
    with pytest.raises(ValueError, match="norm_method"):
        m(torch.zeros(3, 6), [[0], [1, 2], []], [[1.0], [1.0, 2.0], []])


def test_cpu_tensors_keep_the_torch_code_under_either_setting():
    """features on the CPU never take the kernel path, so "hip" and "torch" run the same code there and give the same bits for
    the output and every gradient (tests/test_hip_layer_norm.py runs both on a machine with a device: the pooling needs one)"""
    from model.aggregators import ImportanceAggregator
    m = ImportanceAggregator(6, 4)
    x = torch.randn(5, 6)
    for method in ("hip", "torch"):
        m.norm_method = method
        assert not m._hip_norm(x)
        assert not m._hip_norm(x.double()) and not m._hip_norm(x[0])


def test_layer_norm_torch_is_layer_norm_and_where():
    from pinsage_hip import dense
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 12, generator=g, requires_grad=True)
    gamma, beta = torch.randn(12, generator=g, requires_grad=True), torch.randn(12, generator=g, requires_grad=True)
    live = torch.tensor([1, 0, 3, -1, 1, 1, 0], dtype=torch.int32)
    y = dense.layer_norm(x, gamma, beta, 1e-5, live)                  # CPU tensors: the torch expression
    ref = torch.nn.functional.layer_norm(x, (12,), gamma, beta, 1e-5)
    ref = torch.where((live > 0)[:, None], ref, torch.zeros_like(ref))
    assert torch.equal(y, ref) and y.requires_grad
    assert torch.equal(dense.layer_norm(x, gamma, beta), torch.nn.functional.layer_norm(x, (12,), gamma, beta, 1e-5))
