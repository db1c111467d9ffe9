"""model.layers on the device: the two batch-norm entry points (csrc/batch_norm.hip: ps_bn_batch_stats, ps_bn_apply) against the
float64 restatement of tests/helpers/layers_cases.py over its shape table, GraphConvLayer and the three pooling layers against the
reference's recorded outputs (reference_golden_layers.npz) -- never another GPU run.  Layer outputs are held to
rtol 1e-5 / atol 2e-6 (tests/test_hip_model.py's embedding tolerance), maxima to equality; the statistics to the worst-case bound
of an fp64 summation plus the final rounding, with u = 2^-53 and S the partition length:

  mean    |err| <= (2^-23 + 2 M u) |mean|
  var     |err| <= 2^-23 var + 2 M u E[z^2]          (relative: 2^-23 + 2 M u kappa, kappa = E[z^2] / var)
  scale   gamma / sqrt(var + eps): half the relative error of var + eps, plus one rounding of the result and one of eps to fp32
  running statistics  (1 - m) old + m new: m times the bound of `new`, plus 2^-22 of the two terms' magnitudes (the rounding of
          the result, and of m and 1 - m to fp32)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import layers_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = lc.RTOL, lc.ATOL
U = 2.0 ** -53
SHAPES = [(M, N, 0) for M in lc.STATS_M for N in lc.STATS_N] + [lc.OFFSET_SHAPE + (1,)]
SHAPE_IDS = [f"M{M}-N{N}" + ("-offset" if o else "") for M, N, o in SHAPES]


def _dev(a, offset=0):
    """a on the device; offset: that many elements into its storage (contiguous, not 16-byte aligned for one float)"""
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.tensor(a).cuda()
    buf = torch.empty(a.size + offset, dtype=torch.tensor(a[:0]).dtype, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.tensor(a))
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t


def _raw_stats(z, gamma, rm, rv, ws, wsb=None):
    """ps_bn_batch_stats with a workspace of the caller's; returns (rc, mean, var, scale)"""
    from pinsage_hip import native as nv
    M, N = z.shape
    mean, var, scale = (torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(3))
    rc = nv.lib().ps_bn_batch_stats(nv.ptr(z), M, N, nv.ptr(gamma), lc.EPS, lc.MOMENTUM, nv.ptr(rm), nv.ptr(rv), nv.ptr(mean),
                                    nv.ptr(var), nv.ptr(scale), nv.ptr(ws), ws.numel() if wsb is None else wsb, nv.stream())
    return rc, mean, var, scale


def test_partition_length_is_the_helpers():
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    fn = nv.lib().ps_bn_stats_workspace_bytes
    assert dense.BN_STATS_ROWS == lc.S
    assert fn(lc.S, 1) == 16 and fn(lc.S + 1, 1) == 32 and fn(70 * lc.S + 3, 260) == 71 * 2 * 260 * 8
    assert fn(1, 8) == 0 and fn(2, 0) == 0


@pytest.mark.parametrize("M,N,off", SHAPES, ids=SHAPE_IDS)
def test_bn_batch_stats(M, N, off):
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    c = lc.stats_case(M, N)
    ref = lc.bn_stats_ref(c["z"], c["gamma"], c["rm0"], c["rv0"])
    z, gamma = _dev(c["z"], off), _dev(c["gamma"])
    rm, rv = _dev(c["rm0"]), _dev(c["rv0"])
    mean, var, scale = dense.batch_norm_stats(z, gamma, lc.EPS, lc.MOMENTUM, rm, rv)
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in (("mean", mean), ("var", var), ("scale", scale), ("rm", rm), ("rv", rv))}
    mean_tol = (2.0 ** -23 + 2 * M * U) * np.abs(ref["mean"])
    var_tol = 2.0 ** -23 * ref["var"] + 2 * M * U * ref["ez2"]
    scale_tol = np.abs(ref["scale"]) * (2.0 ** -23 + 0.5 * var_tol / (ref["var"] + lc.EPS))
    m = lc.MOMENTUM
    rm_tol = m * mean_tol + 2.0 ** -22 * ((1 - m) * np.abs(c["rm0"]) + m * np.abs(ref["mean"]))
    rv_tol = m * var_tol * M / (M - 1) + 2.0 ** -22 * ((1 - m) * np.abs(c["rv0"]) + m * ref["var"] * M / (M - 1))
    err = {k: np.abs(got[k] - ref[k]) for k in got}
    kappa = ref["ez2"][0] / ref["var"][0]
    print(f"M {M} N {N}: max err / bound  mean {np.max(err['mean'] / mean_tol):.3f}  var {np.max(err['var'] / np.maximum(var_tol, 1e-300)):.3f}"
          f"  scale {np.max(err['scale'] / scale_tol):.3f}  rm {np.max(err['rm'] / rm_tol):.3f}  rv {np.max(err['rv'] / rv_tol):.3f}"
          f"  | planted column: kappa {kappa:.2e}, rel var err {err['var'][0] / ref['var'][0]:.2e}")
    assert (got["var"] >= 0).all()
    for k, tol in (("mean", mean_tol), ("var", var_tol), ("scale", scale_tol), ("rm", rm_tol), ("rv", rv_tol)):
        assert (err[k] <= tol).all(), (k, int(np.argmax(err[k] - tol)), float(np.max(err[k] - tol)))
    if M >= 3:
        assert kappa > 1e5                                   # the planted column is what it claims to be
    if N >= 2:                                               # the constant column
        assert 0 <= got["var"][N - 1] <= 2 * M * U * float(lc.CONST) ** 2 and got["mean"][N - 1] == float(lc.CONST)
    # the same bits again, and once more from a workspace full of 0xFF bytes (NaNs, as doubles)
    mean2, var2, scale2 = dense.batch_norm_stats(z, gamma, lc.EPS, lc.MOMENTUM)
    assert torch.equal(mean, mean2) and torch.equal(var, var2) and torch.equal(scale, scale2)
    assert np.array_equal(rm.cpu().numpy().astype(np.float64), got["rm"])          # no running pointers: no update
    wsb = nv.lib().ps_bn_stats_workspace_bytes(M, N)
    ws = torch.full((wsb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    rc, mean3, var3, scale3 = _raw_stats(z, gamma, None, None, ws)
    assert rc == nv.PS_OK
    assert torch.equal(mean, mean3) and torch.equal(var, var3) and torch.equal(scale, scale3)
    assert (ws[wsb:] == 0xFF).all()                          # nothing is written past the workspace's size


def test_bn_batch_stats_refuses():
    from pinsage_hip import native as nv
    c = lc.stats_case(3, 21)
    z, gamma, rm, rv = _dev(c["z"]), _dev(c["gamma"]), _dev(c["rm0"]), _dev(c["rv0"])
    wsb = nv.lib().ps_bn_stats_workspace_bytes(3, 21)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    assert _raw_stats(z, gamma, rm, rv, ws)[0] == nv.PS_OK
    assert _raw_stats(z[:1], gamma, rm, rv, ws)[0] == nv.PS_EINVAL                # M = 1
    assert _raw_stats(z, gamma, rm, rv, ws, wsb - 1)[0] == nv.PS_EINVAL            # a short workspace
    assert _raw_stats(z, gamma, rm, None, ws)[0] == nv.PS_EINVAL                   # one running pointer alone
    assert _raw_stats(z, gamma, None, rv, ws)[0] == nv.PS_EINVAL
    assert _raw_stats(z, None, rm, rv, ws)[0] == nv.PS_EINVAL
    torch.cuda.synchronize()
    ref = lc.bn_stats_ref(c["z"], c["gamma"], c["rm0"], c["rv0"])
    np.testing.assert_allclose(rv.cpu().numpy(), ref["rv"], rtol=1e-6)              # the refused calls changed nothing: one update
    np.testing.assert_allclose(rm.cpu().numpy(), ref["rm"], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("M,N,off", SHAPES, ids=SHAPE_IDS)
def test_bn_apply(M, N, off):
    from pinsage_hip import dense
    c = lc.stats_case(M, N)
    zh = c["z"].copy()
    zh[c["neg_row"]] = c["neg"]
    z = _dev(zh, off)
    mean, scale, beta = _dev(c["ap_mean"], off), _dev(c["ap_scale"], off), _dev(c["beta"], off)
    for relu in (False, True):
        for l2 in (False, True):
            ref = lc.bn_apply_ref(zh, c["ap_mean"], c["ap_scale"], c["beta"], relu, l2)
            out = dense.batch_norm_apply(z, mean, scale, beta, relu, l2)
            got = out.cpu().numpy()
            print(f"M {M} N {N} relu {relu} l2 {l2}: max |y - ref| {np.abs(got - ref).max():.2e}")
            assert got.shape == ref.shape and got.dtype == np.float32
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
            if relu:                                          # exactly +0.0: no NaN, no -0.0
                row = got[c["neg_row"]]
                assert not row.any() and not np.signbit(row).any()
            else:
                assert (got[c["neg_row"]] < 0).all()
            z2 = z.clone() if not off else _dev(zh, off)
            assert dense.batch_norm_apply(z2, mean, scale, beta, relu, l2, out=z2) is z2
            assert torch.equal(z2, out)                       # in place: the bits of out of place
    assert torch.equal(z.cpu(), torch.tensor(zh))             # out of place leaves z alone


def test_bn_apply_empty_and_refusals():
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    z = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    v = torch.zeros(8, dtype=torch.float32, device="cuda")
    assert dense.batch_norm_apply(z, v, v, v, True, True).shape == (0, 8)
    fn = nv.lib().ps_bn_apply
    assert fn(None, 0, 8, None, None, None, 3, None, nv.stream()) == nv.PS_OK
    z = torch.ones((2, 8), dtype=torch.float32, device="cuda")
    assert fn(nv.ptr(z), 2, 0, nv.ptr(v), nv.ptr(v), nv.ptr(v), 3, nv.ptr(z), nv.stream()) == nv.PS_EINVAL
    assert fn(nv.ptr(z), 2, 8, nv.ptr(v), None, nv.ptr(v), 3, nv.ptr(z), nv.stream()) == nv.PS_EINVAL
    assert fn(nv.ptr(z), 2, 8, nv.ptr(v), nv.ptr(v), nv.ptr(v), 3, None, nv.stream()) == nv.PS_EINVAL
    torch.cuda.synchronize()
    assert (z == 1).all()


# ---- GraphConvLayer --------------------------------------------------------------------------------------------------------------
def _layer(prefix, cin, cout):
    from model import layers as L
    m = L.GraphConvLayer(cin, cout)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in lc.state_dict(prefix).items()}, strict=True)
    return m.cuda()


def _close(got, want):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want, rtol=RTOL, atol=ATOL)


class _Spy:
    """records the names nv.call is asked for"""

    def __init__(self, monkeypatch):
        from pinsage_hip import native as nv
        self.names = []
        real = nv.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(nv, "call", call)

    def take(self):
        names, self.names = self.names, []
        return names


def test_graph_conv_layer_golden(monkeypatch):
    g = lc.golden()
    spy = _Spy(monkeypatch)
    xa, na, xb, nb = (_dev(g[k]) for k in ("x_a", "n_a", "x_b", "n_b"))
    with torch.no_grad():
        m = _layer("p_", 40, 48).train()
        out = m(xa, na)
        assert "ps_bn_batch_stats" in spy.take() and not out.requires_grad
        _close(out, g["out_a"])
        _close(m.bn.running_mean, g["rm_1"])
        _close(m.bn.running_var, g["rv_1"])
        _close(m(xb, nb), g["out_b"])
        _close(m.bn.running_mean, g["rm_2"])
        _close(m.bn.running_var, g["rv_2"])
        assert int(m.bn.num_batches_tracked) == 2
        spy.take()
        m.eval()
        _close(m(xa, na), g["out_eval"])
        assert set(spy.take()) == {"ps_linear"}               # eval: batch norm is folded into the weights
        _close(m.bn.running_var, g["rv_2"])
        assert int(m.bn.num_batches_tracked) == 2


def test_graph_conv_layer_small_batches(monkeypatch):
    g = lc.golden()
    xa, na = _dev(g["x_a"]), _dev(g["n_a"])
    with torch.no_grad():
        m = _layer("p_", 40, 48).train()
        _close(m(xa[:2], na[:2]), g["out_m2"])
        _close(m.bn.running_mean, g["rm_m2"])
        _close(m.bn.running_var, g["rv_m2"])
        assert int(m.bn.num_batches_tracked) == 1
        for mode in (True, False):
            m = _layer("p_", 40, 48).train(mode)
            spy = _Spy(monkeypatch)
            _close(m(xa[:1], na[:1]), g["out_m1"])            # one row: no batch norm in either mode, buffers untouched
            assert set(spy.take()) == {"ps_linear"}
            assert int(m.bn.num_batches_tracked) == 0 and not m.bn.running_mean.any() and (m.bn.running_var == 1).all()
            out = m(xa[:0], na[:0])
            assert out.shape == (0, 48) and out.is_cuda and out.dtype == torch.float32 and not spy.take()
            assert int(m.bn.num_batches_tracked) == 0


def test_graph_conv_layer_ragged():
    """(193, 33 -> 21): no dimension a multiple of four, the scalar sweeps of both kernels"""
    g = lc.golden()
    x, n = _dev(g["r_x"]), _dev(g["r_n"])
    with torch.no_grad():
        m = _layer("r_", 33, 21).train()
        _close(m(x, n), g["r_out_train"])
        _close(m.bn.running_mean, g["r_rm"])
        _close(m.bn.running_var, g["r_rv"])
        _close(m.eval()(x, n), g["r_out_eval"])


def test_graph_conv_layer_dispatch(monkeypatch):
    g = lc.golden()
    xa, na = _dev(g["x_a"]), _dev(g["n_a"])
    spy = _Spy(monkeypatch)
    m = _layer("p_", 40, 48).train()
    out = m(xa, na)                                           # grad mode on, parameters require grad: the torch path
    assert not spy.take() and out.requires_grad
    _close(out, g["out_a"])
    _close(m.bn.running_var, g["rv_1"])
    out.square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert m.linear_self.weight.grad.abs().sum() > 0 and m.bn.weight.grad.abs().sum() > 0
    with torch.no_grad():
        m = _layer("p_", 40, 48).train()
        m.bn.momentum = None                                  # cumulative average: not the default configuration
        out = m(xa, na)
        assert not spy.take()
        _close(out, g["out_a"])                               # the normalisation itself does not depend on the momentum
        assert int(m.bn.num_batches_tracked) == 1
        m = _layer("p_", 40, 48).double().train()
        assert m(xa.double(), na.double()).dtype == torch.float64 and not spy.take()
    # frozen parameters and plain inputs: the kernels, with grad mode on
    m = _layer("p_", 40, 48).train()
    for p in m.parameters():
        p.requires_grad_(False)
    _close(m(xa, na), g["out_a"])
    assert "ps_bn_batch_stats" in spy.take()


def test_graph_conv_layer_peak_memory():
    """M = 16 384, 256 -> 256, training mode: one [M, O] buffer (the apply step runs in place) plus the composed weights and the
    statistics workspace"""
    from model import layers as L
    from pinsage_hip import native as nv
    M, C = 16384, 256
    torch.manual_seed(3)
    m = L.GraphConvLayer(C, C).cuda().train()
    x, n = torch.randn(M, C, device="cuda"), torch.randn(M, C, device="cuda")
    with torch.no_grad():
        m(x[:256], n[:256])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = m(x, n)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - base
    limit = int(1.5 * M * C * 4) + nv.lib().ps_bn_stats_workspace_bytes(M, C)
    print(f"peak allocation above the inputs: {grew} bytes, limit {limit}, one [M, O] buffer {M * C * 4}")
    assert out.shape == (M, C) and grew <= limit
    nrm = out.double().norm(dim=1)
    assert ((nrm - 1).abs() < 1e-5).all()


# ---- pooling layers --------------------------------------------------------------------------------------------------------------
def test_pooling_layers_golden(monkeypatch):
    from model import layers as L
    g = lc.golden()
    nb, w = lc.golden_lists()
    short = int(g["pool_short"])
    x = _dev(g["pool_x"])
    imp, wm, mx = L.ImportancePoolingLayer(), L.WeightedMeanPoolingLayer(), L.MaxPoolingLayer()
    spy = _Spy(monkeypatch)
    _close(imp(x, nb, w), g["importance"])
    _close(imp(x, nb, w[:short]), g["importance_short"])
    _close(wm(x, nb, w), g["wmean"])
    _close(wm(x, nb), g["wmean_none"])
    _close(wm(x, nb, w[:short]), g["wmean_short"])
    assert set(spy.take()) == {"ps_importance_pool"}
    out = mx(x, nb)
    assert spy.take() == ["ps_gather_max"]
    assert np.array_equal(out.cpu().numpy(), g["maxpool"]) and not np.signbit(out.cpu().numpy()[g["pool_len"] == 0]).any()
    # features on the autograd tape: gradients arrive
    xg = x.clone().requires_grad_(True)
    (imp(xg, nb, w).sum() + mx(xg, nb).sum()).backward()
    assert xg.grad is not None and xg.grad.abs().sum() > 0


def test_pooling_layers_errors():
    from model import layers as L
    x = _dev(lc.golden()["pool_x"])
    N = x.size(0)
    for layer, extra in ((L.ImportancePoolingLayer(), ([[1.0, 1.0]],)), (L.WeightedMeanPoolingLayer(), ([[1.0, 1.0]],)),
                         (L.MaxPoolingLayer(), ())):
        with pytest.raises(IndexError):
            layer(x, [[0, -N - 1]], *extra)
        with pytest.raises(RuntimeError, match="non-empty"):
            layer(x, [], *([[]] if extra else []))
