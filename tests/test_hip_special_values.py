"""NaN, infinities, overflow and signed zeros through the dense layers, against the C oracle (the definitions of
include/pinsage_hip.h) word for word, a NaN of any payload where the oracle holds a NaN.  tests/helpers/special_cases.py plants the
values into the smallest case of helpers/gemm_cases.py that reaches each kernel instantiation and tests/test_special_cases.py
proves on the CPU that the plantings produce the classes they are there for, that torch's fp64 expression agrees with the oracle
about them, and that the epilogue's earlier selects (which dropped a NaN) disagree with the table.  Normalised finite outputs keep
gemm_cases.norm_bound(N); nothing else has a tolerance.  Special values go into float operands only, never into an index."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_cases as gc  # noqa: E402
import special_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCH_NAMES = ("PS_GEMM_SHARD", "PS_GEMM_PERSIST", "PS_GEMM_DMA")


def _words(t):
    return t.contiguous().view(torch.int32)


def _bad_on_device(got, want, ref64=None, bound=0.0, limit=8):
    """special_cases.mismatches on the device (the large cases are 25 MB a run): first (row, col, got, want)"""
    assert got.dtype == torch.float32 and got.shape == want.shape, (got.dtype, tuple(got.shape), tuple(want.shape))
    wnan = torch.isnan(want)
    ok = torch.where(wnan, torch.isnan(got), _words(got) == _words(want))
    if ref64 is not None:
        fin = torch.isfinite(want) & (want != 0)
        within = (got.double() - ref64).abs() <= bound * ref64.abs() + 2.0 ** -149
        ok = torch.where(fin, within, ok)
    bad = torch.nonzero(~ok)[:limit].cpu().tolist()
    return [(r, c, float(got[r, c]), float(want[r, c])) for r, c in bad]


_OPS, _WANT = {}, {}


def _device_operands(c, variant):
    """x, W, b, x2, W2 on the device; W / W2 are the views of the case's layout, handed to the kernel without a copy"""
    if (c, variant) not in _OPS:
        d = sc.data(c, variant)
        dev = lambda a: None if a is None else torch.tensor(a).cuda()      # noqa: E731  (a copy: the cached arrays are read-only)
        W = gc.view_of(dev(d.Wbig), c.K, c.layout)
        W2 = None if d.W2big is None else gc.view_of(dev(d.W2big), c.K2, c.layout)
        off, ld = gc.claimed_alignment(c.K, c.layout)
        assert W.data_ptr() % 16 == off and W.stride(0) == ld and W.stride(1) == 1
        _OPS[(c, variant)] = (dev(d.x), W, dev(d.b), dev(d.x2), W2)
    return _OPS[(c, variant)]


def _want(c, variant, relu, l2):
    key = (c, variant, relu, l2)
    if key not in _WANT:
        ref64 = torch.tensor(sc.expected_ref64(c, variant, relu)).cuda() if l2 else None
        _WANT[key] = (torch.tensor(sc.expected(c, variant, relu, l2)).cuda(), ref64)
    return _WANT[key]


def _check_linear(c, variant, env=(), staged=False):
    from pinsage_hip import dense
    x, W, b, x2, W2 = _device_operands(c, variant)
    if staged:
        W, W2 = dense.stage_weight(W), dense.stage_weight(W2)
        assert isinstance(W, dense.StagedWeight) and (W2 is None or isinstance(W2, dense.StagedWeight))
    failures = []
    for (relu, l2) in sc.flagsets_of(c, variant):
        got = dense.linear(x, W, b, x2=x2, W2=W2, relu=relu, l2norm=l2)
        assert tuple(got.shape) == (c.M, c.N)
        want, ref64 = _want(c, variant, relu, l2)
        bad = _bad_on_device(got, want, ref64, gc.norm_bound(c.N))
        kernel = gc.launcher_choice(c.M, c.K, c.N, c.K2, c.layout, l2, env=env, staged=staged)
        print(f"{c.name} {variant} relu={relu} l2={l2} env={dict(env)} staged={staged}: {kernel}: {'ok' if not bad else bad}")
        if bad:
            failures.append(f"case {c.name}, planting {variant}, relu={relu}, l2={l2}, switches {dict(env)}, image-order weights "
                            f"{staged}; expected kernel {kernel}; first (row, col, got, want): {bad}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("c", sc.BASES, ids=lambda c: c.name)
def test_linear_special_values_vs_oracle(c, variant, monkeypatch):
    """every planted case under the launcher's own choice (the N > 256 case: the GEMM, then l2norm_rows_kernel)"""
    for name in SWITCH_NAMES:
        monkeypatch.delenv(name, raising=False)
    _check_linear(c, variant)


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("c", sc.FAST_BASES, ids=lambda c: c.name)
def test_linear_special_values_under_every_launcher_switch(c, variant, monkeypatch):
    """the aligned cases again under gemm_cases.switch_runs: both rings, the one-tile and persistent kernels, the LDS-DMA kernel,
    image-order weights"""
    failures = []
    for env, staged in gc.switch_runs(c):
        for name in SWITCH_NAMES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env:
            monkeypatch.setenv(name, value)
        try:
            _check_linear(c, variant, env=env, staged=staged)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---- ps_gcn_layer ----------------------------------------------------------------------------------------------------------------------
def test_gcn_layer_poison_follows_the_kept_ids(monkeypatch):
    """ps_gcn_layer at its gate (M = 64 * 384 + 37, N = 256, T = 5) with a NaN and a +Inf planted in two rows of h_full: the fused
    layer against the pair it replaces (PS_GCN_FUSED=0), word for word, NaN by class; the output rows that hold a NaN are exactly
    the rows whose kept ids (j < min(nvalid, T), 0 <= id <= max_idx: computed here on the host) include a planted row, and every
    other row has the bits of the run without the plant.  W2 stays finite: "for finite w" is a precondition of the tiles that
    skip the pooled operand (include/pinsage_hip.h, ps_gcn_layer), not something the layer checks."""
    import gcn_cases as gn
    import test_hip_gcn_matrix as gm
    from pinsage_hip import dense
    for name in gm.SWITCH_NAMES:
        monkeypatch.delenv(name, raising=False)
    c = gn._gc("special-k32h64-T5-mixed-counts", gn.RAGGED, 32, 64, 5, "counts", "mixed", renorms=(1,),
               situation="a NaN row and an Inf row of h_full among the gathered rows")
    assert gn.gcn_served(c.M, c.K, 256, c.H, c.T) and c.M == 64 * 384 + 37 and c.T <= 16
    d = gn.gcn_data(c)
    assert bool(np.isfinite(d.W2).all()) and bool((d.W2 != 0).all())
    ids, nvalid = d.rows.ids, d.rows.nvalid
    kept = (np.arange(c.T)[None, :] < np.minimum(nvalid, c.T)[:, None]) & (ids >= 0) & (ids <= d.max_idx)
    freq = np.bincount(ids[kept], minlength=d.n_full)
    p_nan, p_inf = (int(i) for i in np.argsort(-freq, kind="stable")[:2])
    h = d.h_full.copy()
    h[p_nan, 3], h[p_inf, 5] = np.nan, np.inf
    gathers_nan = (kept & (ids == p_nan)).any(axis=1)
    gathers = gathers_nan | (kept & (ids == p_inf)).any(axis=1)
    heavy = kept.any(axis=1)
    assert gathers.sum() >= 2 and (heavy & ~gathers).sum() > 64 and (~heavy).sum() > 64 and gathers_nan.any() and (gathers & ~gathers_nan).any()
    ops = dict(x=gm._dev(d.x), W=gm._dev(d.W), b=gm._dev(d.b), ids=gm._dev(ids), counts=gm._dev(d.rows.counts), wts=None,
               nvalid=gm._dev(nvalid), W2=gm._dev(d.W2), max_idx=d.max_idx_arg)
    clean = gm._fused(**ops, h_full=gm._dev(d.h_full), renorm=1)
    fused = gm._fused(**ops, h_full=gm._dev(h), renorm=1)
    monkeypatch.setenv("PS_GCN_FUSED", "0")
    pair = dense.gcn_layer(ops["x"], ops["W"], ops["b"], gm._dev(h), ops["ids"], ops["counts"], ops["nvalid"], ops["W2"],
                           max_idx=ops["max_idx"], renorm=True)
    bad = _bad_on_device(fused, pair)                                        # a NaN equals any NaN, else the uint32 words
    assert not bad, f"fused against PS_GCN_FUSED=0, first (row, col, got, want): {bad}"
    got = fused.cpu().numpy()
    poisoned = np.isnan(got).any(axis=1)
    assert np.array_equal(poisoned, gathers), (f"rows with a NaN that gather no planted row: {np.flatnonzero(poisoned & ~gathers)[:8]}; "
                                               f"rows that gather one and hold no NaN: {np.flatnonzero(gathers & ~poisoned)[:8]}")
    assert bool(np.isnan(got[gathers_nan]).all())                          # NaN * w2 in every column
    ok = ~gathers
    assert np.array_equal(got[ok].view(np.uint32), clean.cpu().numpy()[ok].view(np.uint32)), "a row beside the poisoned ones changed"


# ---- the backward: ps_linear_epilogue_bwd, ps_linear_wgrad, LinearFn, PinSage -------------------------------------------------------------
@pytest.mark.parametrize("relu,l2", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("N", sc.EPI_N)
def test_epilogue_bwd_special_values(N, relu, l2):
    """the planted activations of special_cases.epilogue_special against the restatement bit for bit (a NaN equals any NaN), and
    against torch's fp64 autograd by class (one named deviation: special_cases.epilogue_class_mismatches)"""
    from helpers import linear_bwd_cases as lb
    from pinsage_hip import dense
    t, g, rows = sc.epilogue_special(N)
    gz = dense.linear_epilogue_bwd(torch.tensor(t).cuda(), torch.tensor(g).cuda(), relu, l2).cpu().numpy()
    bad = lb.mismatches(gz, lb.epilogue_bwd_exact(t, g, relu, l2, lb.vec_of(N)))
    assert bad == [], f"N={N} relu={relu} l2={l2} rows {rows}: first (row, col, got, want) {bad}"
    bad = sc.epilogue_class_mismatches(gz, t, g, relu, l2)
    assert bad == [], f"N={N} relu={relu} l2={l2} rows {rows}: first (row, col, class, torch's class) {bad}"


def test_wgrad_poison_stays_in_its_column():
    """a NaN in g[r, n]: row n of dW and db[n] are NaN, as g.T @ x gives it in fp64; everything else has the bits of the run
    without the plant"""
    from helpers import linear_bwd_cases as lb
    from pinsage_hip import dense
    N, K = lb.WGRAD_SHAPES[1]
    P = lb.partition(1)
    M = P + 1
    g, x = lb.wgrad_data(M, N, K, lb.partition(M))
    r, n = P - 3, 7
    gp = g.copy()
    gp[r, n] = np.nan
    dW0, db0 = (a.cpu().numpy() for a in dense.linear_wgrad(torch.tensor(g).cuda(), torch.tensor(x).cuda()))
    dW, db = (a.cpu().numpy() for a in dense.linear_wgrad(torch.tensor(gp).cuda(), torch.tensor(x).cuda()))
    want = np.isnan(gp.astype(np.float64).T @ x.astype(np.float64))
    assert want[n].all() and want.sum() == K
    assert np.array_equal(np.isnan(dW), want) and np.array_equal(np.isnan(db), np.arange(N) == n)
    rest = np.arange(N) != n
    assert np.array_equal(dW[rest].view(np.uint32), dW0[rest].view(np.uint32)) and np.array_equal(db[rest].view(np.uint32), db0[rest].view(np.uint32))


@pytest.mark.parametrize("relu,l2", [(False, False), (True, False), (False, True), (True, True)])
def test_linear_on_the_tape_with_a_poisoned_row(relu, l2, monkeypatch):
    """LinearFn with x2 / W2 at the shape of test_linear_is_differentiable, a NaN in one row of x.  The training forward equals the
    inference call on the poisoned row too (the bits before the norm; after it a NaN where the inference call holds one and
    gemm_cases.norm_bound elsewhere).  Without the ReLU every gradient has the class it has under grad_method = "torch"; with it
    the header's mask (t > 0) zeroes the poisoned row's gradient where torch passes it on (special_cases: MASK_NAN), so only the
    rows of dx beside it are compared."""
    from helpers import linear_bwd_cases as lb
    from pinsage_hip import dense, sampling
    M = lb.partition(1) + 40
    d = dict(lb.layer_data(M, 16, 12, 8))
    r = 3
    d["x"] = d["x"].copy()
    d["x"][r, 15] = np.nan
    leaves = ("x", "W", "b", "x2", "W2")
    G = torch.tensor(d["G"]).cuda()

    def step():
        ls = {k: torch.tensor(d[k]).cuda().requires_grad_(True) for k in leaves}
        y = dense.linear(ls["x"], ls["W"], ls["b"], x2=ls["x2"], W2=ls["W2"], relu=relu, l2norm=l2)
        y.backward(G)
        return y.detach(), {k: ls[k].grad.cpu().numpy() for k in leaves}
    with torch.no_grad():
        ops = {k: torch.tensor(d[k]).cuda() for k in leaves}
        y_inf = dense.linear(ops["x"], ops["W"], ops["b"], x2=ops["x2"], W2=ops["W2"], relu=relu, l2norm=l2)
        t_inf = dense.linear(ops["x"], ops["W"], ops["b"], x2=ops["x2"], W2=ops["W2"], relu=relu)
    assert bool(torch.isnan(y_inf[r]).all()) and not bool(torch.isnan(y_inf[torch.arange(M) != r]).any())
    y, grads = step()
    with np.errstate(invalid="ignore"):
        ref64 = gc.ref_normed(t_inf.cpu().numpy()) if l2 else None
    bad = sc.mismatches(y.cpu().numpy(), y_inf.cpu().numpy(), ref64)
    assert bad == [], f"relu={relu} l2={l2}: training forward against the inference call, first (row, col, got, want) {bad}"
    monkeypatch.setattr(sampling, "grad_method", "torch")
    y_t, grads_t = step()
    monkeypatch.setattr(sampling, "grad_method", "hip")
    assert np.array_equal(np.isnan(y_t.cpu().numpy()), np.isnan(y.cpu().numpy()))
    for k in leaves:
        got, want = sc.classes(grads[k]), sc.classes(grads_t[k])
        if not relu:
            assert np.array_equal(got, want), (k, relu, l2, np.argwhere(got != want)[:8].tolist())
        elif k in ("x", "x2"):
            rest = np.arange(M) != r
            assert np.array_equal(got[rest], want[rest]), (k, relu, l2)


def _pinsage_case(branch):
    import test_hip_linear_bwd as tl
    x, kw = tl._model_case(branch)
    xp = x.clone()
    xp[17, 3] = float("nan")
    return x, xp, kw


@pytest.mark.parametrize("branch", ["mlp", "edge", "pooled"])
def test_pinsage_branch_with_a_poisoned_feature_row(branch, monkeypatch):
    """16 -> 32 -> 8, two layers, 300 rows (test_pinsage_branch_takes_a_training_step's), one NaN among the features.  The
    inference output and the training forward hold a NaN exactly where the torch layers (grad_method = "torch") put one, and every
    other row has the bits of the run without the NaN.  The gradients are not compared: every hidden layer has a ReLU, whose
    backward mask (t > 0) differs from torch's at a NaN activation by the header's definition (special_cases: MASK_NAN)."""
    import model.pinsage as pin
    from pinsage_hip import sampling
    torch.manual_seed(7)
    model = pin.PinSage(16, 32, 8, 2).cuda()
    x, xp, kw = _pinsage_case(branch)
    monkeypatch.setattr(sampling, "grad_method", "torch")
    want = torch.isnan(model(xp, **kw).detach()).cpu().numpy()
    monkeypatch.setattr(sampling, "grad_method", "hip")
    rows = want.any(axis=1)
    assert rows[17] and 0 < rows.sum() < 300 and np.array_equal(want, np.repeat(rows[:, None], 8, axis=1))
    assert (rows.sum() == 1) == (branch == "mlp")
    with torch.no_grad():
        runs = {"inference": (model(xp, **kw), model(x, **kw))}
    runs["training forward"] = (model(xp, **kw).detach(), model(x, **kw).detach())
    for what, (got, clean) in runs.items():
        got, clean = got.cpu().numpy(), clean.cpu().numpy()
        assert np.array_equal(np.isnan(got), want), (branch, what, np.flatnonzero(np.isnan(got).any(axis=1) != rows)[:8])
        assert np.array_equal(got[~rows].view(np.uint32), clean[~rows].view(np.uint32)), (branch, what)
