"""model.layers without a GPU: the float64 restatement of tests/helpers/layers_cases.py against the reference's float64 outputs
(1e-12), and the drop-in classes on CPU tensors (their torch path) against its fp32 outputs at the embedding tolerance; a
reference state_dict loads strictly and a freshly seeded layer has the reference's initial parameters."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import layers_cases as lc  # noqa: E402

RTOL, ATOL = lc.RTOL, lc.ATOL
BUFFERS = ("bn.running_mean", "bn.running_var", "bn.num_batches_tracked")


def _close64(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_restatement_graph_conv_float64():
    g = lc.golden()
    sd = lc.state_dict("p_")
    out, s1 = lc.graph_conv_ref(sd, g["x_a"], g["n_a"], True)
    _close64(out, g["out_a64"])
    _close64(s1["bn.running_mean"], g["rm_164"])
    _close64(s1["bn.running_var"], g["rv_164"])
    out, s2 = lc.graph_conv_ref(s1, g["x_b"], g["n_b"], True)
    _close64(out, g["out_b64"])
    _close64(s2["bn.running_mean"], g["rm_264"])
    _close64(s2["bn.running_var"], g["rv_264"])
    assert int(s2["bn.num_batches_tracked"]) == int(g["nbt_264"]) == 2
    out, s3 = lc.graph_conv_ref(s2, g["x_a"], g["n_a"], False)
    _close64(out, g["out_eval64"])
    assert all(np.array_equal(s3[k], s2[k]) for k in BUFFERS)
    out, s = lc.graph_conv_ref(sd, g["x_a"][:2], g["n_a"][:2], True)        # M = 2: the unbiased factor is 2
    _close64(out, g["out_m264"])
    _close64(s["bn.running_var"], g["rv_m264"])
    _close64(s["bn.running_mean"], g["rm_m264"])
    out, s = lc.graph_conv_ref(sd, g["x_a"][:1], g["n_a"][:1], True)        # M = 1: no batch norm
    _close64(out, g["out_m164"])
    assert int(s["bn.num_batches_tracked"]) == int(g["nbt_m164"]) == 0 and not s["bn.running_mean"].any()
    rd = lc.state_dict("r_")
    out, s = lc.graph_conv_ref(rd, g["r_x"], g["r_n"], True)
    _close64(out, g["r_out_train64"])
    _close64(s["bn.running_mean"], g["r_rm64"])
    _close64(s["bn.running_var"], g["r_rv64"])
    _close64(lc.graph_conv_ref(s, g["r_x"], g["r_n"], False)[0], g["r_out_eval64"])


def test_restatement_pooling_float64():
    g = lc.golden()
    nb, w = lc.golden_lists()
    short = int(g["pool_short"])
    x = g["pool_x"]
    _close64(lc.importance_pool_ref(x, nb, w), g["importance64"])
    _close64(lc.importance_pool_ref(x, nb, w[:short]), g["importance_short64"])
    _close64(lc.weighted_mean_pool_ref(x, nb, w), g["wmean64"])
    _close64(lc.weighted_mean_pool_ref(x, nb), g["wmean_none64"])
    _close64(lc.weighted_mean_pool_ref(x, nb, w[:short]), g["wmean_short64"])
    assert np.array_equal(lc.max_pool_ref(x.astype(np.float64), nb), g["maxpool64"])
    assert np.array_equal(lc.max_pool_ref(x, nb), g["maxpool"])
    # the cases are what they claim to be: the misaligned weights matter, and so do the rows past the short weight list
    assert g["importance_short64"].shape[0] == short < len(nb)
    assert np.abs(g["wmean_short64"][short:] - g["wmean64"][short:]).max() > 1e-3
    aligned = x[[3, 7, 9]].astype(np.float64).T @ (np.array([0.1, 0.3, 0.4]) / 0.8)
    assert np.abs(g["importance64"][5] - aligned).max() > 1e-3


def _layer(prefix, cin, cout):
    from model import layers as L
    m = L.GraphConvLayer(cin, cout)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in lc.state_dict(prefix).items()}, strict=True)
    return m


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _close(got, want):
    np.testing.assert_allclose(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, want, rtol=RTOL, atol=ATOL)


def test_state_dict_loads_and_initial_parameters_match():
    from model import layers as L
    g = lc.golden()
    torch.manual_seed(int(g["seed"]))
    m = L.GraphConvLayer(40, 48)
    init = lc.state_dict("init_")
    sd = m.state_dict()
    assert list(sd) == list(init) or sorted(sd) == sorted(init)
    for k, v in init.items():
        assert sd[k].dtype == _t(v).dtype and np.array_equal(sd[k].numpy(), v), k
    assert not m.linear_self.bias.any() and not m.linear_out.bias.any()
    m.load_state_dict({k: _t(v) for k, v in lc.state_dict("p_").items()}, strict=True)
    assert isinstance(m.bn, torch.nn.BatchNorm1d) and m.bn.eps == lc.EPS and m.bn.momentum == lc.MOMENTUM
    assert m.linear_out.in_features == 96 and m.linear_neigh.in_features == 40


def test_graph_conv_cpu_matches_the_reference():
    g = lc.golden()
    with torch.no_grad():
        m = _layer("p_", 40, 48).train()
        _close(m(_t(g["x_a"]), _t(g["n_a"])), g["out_a"])
        _close(m.bn.running_mean, g["rm_1"])
        _close(m.bn.running_var, g["rv_1"])
        _close(m(_t(g["x_b"]), _t(g["n_b"])), g["out_b"])
        _close(m.bn.running_mean, g["rm_2"])
        _close(m.bn.running_var, g["rv_2"])
        assert int(m.bn.num_batches_tracked) == 2
        m.eval()
        _close(m(_t(g["x_a"]), _t(g["n_a"])), g["out_eval"])
        assert int(m.bn.num_batches_tracked) == 2
        m = _layer("p_", 40, 48).train()
        _close(m(_t(g["x_a"][:2]), _t(g["n_a"][:2])), g["out_m2"])
        _close(m.bn.running_var, g["rv_m2"])
        m = _layer("p_", 40, 48).train()
        _close(m(_t(g["x_a"][:1]), _t(g["n_a"][:1])), g["out_m1"])
        assert int(m.bn.num_batches_tracked) == 0 and not m.bn.running_mean.any() and (m.bn.running_var == 1).all()
        m = _layer("r_", 33, 21).train()
        _close(m(_t(g["r_x"]), _t(g["r_n"])), g["r_out_train"])
        _close(m.bn.running_mean, g["r_rm"])
        _close(m.bn.running_var, g["r_rv"])
        _close(m.eval()(_t(g["r_x"]), _t(g["r_n"])), g["r_out_eval"])
        # float64 modules run the same code
        m = _layer("p_", 40, 48).double().train()
        np.testing.assert_allclose(m(_t(g["x_a"]).double(), _t(g["n_a"]).double()).numpy(), g["out_a64"], rtol=1e-10, atol=1e-12)


def test_graph_conv_cpu_is_differentiable():
    g = lc.golden()
    m = _layer("p_", 40, 48).train()
    out = m(_t(g["x_a"]), _t(g["n_a"]))
    assert out.requires_grad
    out.square().sum().backward()
    _close(out, g["out_a"])
    assert all(p.grad is not None for p in m.parameters())


def test_pooling_layers_cpu_match_the_reference():
    from model import layers as L
    g = lc.golden()
    nb, w = lc.golden_lists()
    short = int(g["pool_short"])
    x = _t(g["pool_x"])
    imp, wm, mx = L.ImportancePoolingLayer(), L.WeightedMeanPoolingLayer(), L.MaxPoolingLayer()
    assert not list(imp.parameters()) and not list(wm.parameters()) and not list(mx.parameters())
    _close(imp(x, nb, w), g["importance"])
    _close(imp(x, nb, w[:short]), g["importance_short"])
    _close(wm(x, nb, w), g["wmean"])
    _close(wm(x, nb), g["wmean_none"])
    _close(wm(x, nb, w[:short]), g["wmean_short"])
    assert np.array_equal(mx(x, nb).numpy(), g["maxpool"])
    np.testing.assert_allclose(imp(x.double(), nb, w).numpy(), g["importance64"], rtol=1e-10, atol=1e-12)


def test_pooling_layers_raise_what_the_reference_raises():
    from model import layers as L
    x = _t(lc.golden()["pool_x"])
    N = x.size(0)
    for layer, extra in ((L.ImportancePoolingLayer(), ([[1.0, 1.0]],)), (L.WeightedMeanPoolingLayer(), ([[1.0, 1.0]],)),
                         (L.MaxPoolingLayer(), ())):
        with pytest.raises(IndexError):
            layer(x, [[0, -N - 1]], *extra)
        assert layer(x, [[0, -N]], *extra).shape == (1, x.size(1))
        with pytest.raises(RuntimeError, match="non-empty"):
            layer(x, [], *([[]] if extra else []))
