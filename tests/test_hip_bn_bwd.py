"""ps_bn_bwd (csrc/batch_norm_bwd.hip) on the device against the exact restatement of tests/helpers/bn_bwd_cases.py, bit for bit,
over its case table and the four flag sets; the aliasing, NULL-output and error contracts of include/pinsage_hip.h;
dense.batch_norm on and off the autograd tape; and model.layers.GraphConvLayer with grad_method = "hip".

Bounds.  dense.batch_norm's gradients are held to bn_bwd_cases.bn_bwd_bound (derived in that module's docstring) against the
float64 closed form at the statistics the kernel computed.  GraphConvLayer's gradients are measured against float64 autograd of
`_forward_torch` on a .double() copy: per tensor max |got - ref64| / max |ref64|, and for the three linear biases -- whose exact
gradient is zero, batch norm removes a bias added before it -- the residual over the largest column of sum_r |dL/dz| (float64).
The limit is 4 x the same metric of fp32 `_forward_torch` on the same inputs (the composed map rounds in another order than the
three-GEMM form), never a figure taken from the code under test.  Both values are printed per tensor; DESIGN.md ("Batch-norm
layer, training") records them."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import abi_cases as ac
from helpers import abi_cases_bn_bwd  # noqa: F401  (ps_bn_bwd joins ac.CASES)
from helpers import bn_bwd_cases as bb
from helpers import layers_cases as lc

pytestmark = pytest.mark.gpu
OUT = ("gz", "dgamma", "dbeta")
FLAG_IDS = ["none", "relu", "norm", "relu+norm"]


def _dev(a, offset=0):
    """a on the device; offset: that many elements into its storage (contiguous, not 16-byte aligned for one float)"""
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.tensor(a).cuda()
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.tensor(a))
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t


def _flags(relu, l2):
    from pinsage_hip import native as nv
    return (nv.PS_RELU if relu else 0) | (nv.PS_L2NORM if l2 else 0)


class _Call:
    """one case on the device: the inputs, and ps_bn_bwd with fresh or given outputs"""

    def __init__(self, name, plants=True):
        from pinsage_hip import native as nv
        self.d = d = bb.data(name, plants)
        self.off = bb.case(name)[3]
        self.M, self.N = d["M"], d["N"]
        self.z = _dev(d["z"], self.off)
        self.gy, self.mean, self.var, self.scale, self.beta = (_dev(d[k]) for k in ("gy", "mean", "var", "scale", "beta"))
        self.wsb = nv.lib().ps_bn_bwd_workspace_bytes(self.M, self.N)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")

    def run(self, relu, l2, gz="new", dgamma="new", dbeta="new", gy=None, ws=None, wsb=None, M=None, N=None, z="given",
            flags=None):
        from pinsage_hip import native as nv
        new = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device="cuda")      # noqa: E731
        gz = new(self.M, self.N) if isinstance(gz, str) else gz
        dgamma = new(self.N) if isinstance(dgamma, str) else dgamma
        dbeta = new(self.N) if isinstance(dbeta, str) else dbeta
        gy = self.gy if gy is None else gy
        args = [nv.ptr(self.z if isinstance(z, str) else z), nv.ptr(gy), self.M if M is None else M, self.N if N is None else N,
                nv.ptr(self.mean), nv.ptr(self.var), nv.ptr(self.scale), nv.ptr(self.beta), float(bb.EPS),
                _flags(relu, l2) if flags is None else flags, nv.ptr(gz), nv.ptr(dgamma), nv.ptr(dbeta),
                nv.ptr(self.ws) if ws is None else ws, self.wsb if wsb is None else wsb, nv.stream()]
        rc = nv.lib().ps_bn_bwd(*args)
        torch.cuda.synchronize()
        return rc, dict(gz=gz, dgamma=dgamma, dbeta=dbeta)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what):
    for k in OUT:
        if got[k] is not None and want[k] is not None:
            w = want[k] if isinstance(want[k], np.ndarray) else _np(want[k])
            assert bb.mismatches(_np(got[k]), w) == [], (what, k)


# ---- the kernels against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", bb.FLAGSETS, ids=FLAG_IDS)
@pytest.mark.parametrize("name", bb.NAMES)
def test_kernel_is_the_restatement(name, flags):
    relu, l2 = flags
    c = _Call(name)
    rc, got = c.run(relu, l2)
    assert rc == 0
    _same(got, bb.expected(name, relu, l2), (name, flags))


@pytest.mark.parametrize("flags", bb.FLAGSETS, ids=FLAG_IDS)
@pytest.mark.parametrize("name", ["vec1-2blocks", "vec4-2blocks", "v4-keep", "v4-keep+1", "v1-keep+1", "long"])
def test_gz_may_be_gy_and_outputs_may_be_null(name, flags):
    relu, l2 = flags
    c = _Call(name)
    rc, fresh = c.run(relu, l2)
    assert rc == 0
    gy = c.gy.clone()
    rc, alias = c.run(relu, l2, gz=gy, gy=gy)
    assert rc == 0
    _same(alias, fresh, (name, "in place"))
    for k in OUT:
        rc, part = c.run(relu, l2, **{k: None})
        assert rc == 0 and part[k] is None
        _same(part, fresh, (name, k + " NULL"))
    rc, none = c.run(relu, l2, gz=None, dgamma=None, dbeta=None)
    assert rc == 0


def test_planted_rows_and_columns():
    name = "vec4-2blocks"
    c = _Call(name)
    d = c.d
    _, got = c.run(True, True)
    g0 = d["gamma0_col"]
    assert not got["gz"][:, g0].any() and got["dgamma"][g0] == 0 and got["dbeta"][g0] == 0
    assert torch.isfinite(got["gz"]).all()
    gy2 = c.gy.clone()
    gy2[d["neg_row"]] *= 2.0                                  # a wholly masked row: its gy does not matter
    _, got2 = c.run(True, True, gy=gy2)
    _same(got2, got, "masked row")
    # the rows at the clamp and the row with gy = 0: the restatement decides
    _same(got, bb.expected(name, True, True), "planted")
    e = bb.expected(name, False, False)
    _, plain = c.run(False, False)
    _same(plain, e, "no flags")


def test_error_codes_leave_the_outputs_alone():
    from pinsage_hip import native as nv
    c = _Call("ragged-steps")
    keep = {"ws": c.ws.clone()}

    def untouched(rc, out, code):
        assert rc == code, (rc, code)
        assert all((out[k] == 7).all() for k in OUT)
        assert torch.equal(c.ws, keep["ws"])
    untouched(*c.run(True, True, M=1), nv.PS_EINVAL)
    untouched(*c.run(True, True, N=0), nv.PS_EINVAL)
    untouched(*c.run(True, True, flags=nv.PS_WPERM), nv.PS_EINVAL)
    untouched(*c.run(True, True, flags=8), nv.PS_EINVAL)
    untouched(*c.run(True, True, z=None), nv.PS_EINVAL)
    untouched(*c.run(True, True, ws=ctypes.c_void_p(0)), nv.PS_EINVAL)
    untouched(*c.run(True, True, wsb=c.wsb - 1), nv.PS_EWORKSPACE)
    untouched(*c.run(True, True, ws=ctypes.c_void_p(c.ws.data_ptr() + 4)), nv.PS_EINVAL)
    assert nv.lib().ps_bn_bwd_workspace_bytes(1, 8) == 0 and nv.lib().ps_bn_bwd_workspace_bytes(2, 0) == 0


def test_more_column_blocks_than_a_grid_holds_is_unsupported():
    """N = 65 535 * 64 + 1, VEC 1: one column block more than grid.y takes.  PS_EUNSUPPORTED, and nothing is written."""
    from pinsage_hip import native as nv
    M, N = 2, 65535 * 64 + 1
    z, gy = (torch.zeros((M, N), dtype=torch.float32, device="cuda") for _ in range(2))
    vec = [torch.ones(N, dtype=torch.float32, device="cuda") for _ in range(4)]
    out = [torch.full(s, 7.0, dtype=torch.float32, device="cuda") for s in ((M, N), (N,), (N,))]
    wsb = nv.lib().ps_bn_bwd_workspace_bytes(M, N)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = nv.lib().ps_bn_bwd(nv.ptr(z), nv.ptr(gy), M, N, *(nv.ptr(v) for v in vec), float(bb.EPS), 0, *(nv.ptr(o) for o in out),
                            nv.ptr(ws), wsb, nv.stream())
    torch.cuda.synchronize()
    assert rc == nv.PS_EUNSUPPORTED
    assert all((o == 7).all() for o in out) and (ws == 0xFF).all()


def test_contract_matrix_holds_ps_bn_bwd():
    """The contract matrix of tests/test_hip_abi_contract.py (captured stream, poisoned outputs and workspace, guard bands, replays)
    for ps_bn_bwd, started from here as well: that module parametrises over the case table when it is collected, and a run of it
    alone does not import the case module of this entry point."""
    import test_hip_abi_contract as contract
    assert "ps_bn_bwd" in ac.CASES
    contract.test_contract("ps_bn_bwd")


# ---- dense.batch_norm -----------------------------------------------------------------------------------------------------------
class _Spy:
    """records the names nv.call is asked for"""

    def __init__(self, monkeypatch):
        from pinsage_hip import native as nv
        self.names = []
        real = nv.call

        def call(name, *args, **kw):
            self.names.append(name)
            return real(name, *args, **kw)
        monkeypatch.setattr(nv, "call", call)

    def take(self):
        names, self.names = self.names, []
        return names


def _bn_inputs(name):
    d = bb.data(name, False)
    z, gy, gamma, beta = (_dev(d[k]) for k in ("z", "gy", "gamma", "beta"))
    rm = torch.linspace(-1, 1, d["N"], device="cuda")
    rv = torch.linspace(0.5, 2, d["N"], device="cuda")
    return d, z, gy, gamma, beta, rm, rv


@pytest.mark.parametrize("flags", bb.FLAGSETS, ids=FLAG_IDS)
@pytest.mark.parametrize("name", ["ragged-steps", "vec1-2blocks", "vec4-2blocks"])
def test_dense_batch_norm(name, flags, monkeypatch):
    from pinsage_hip import dense, sampling
    relu, l2 = flags
    monkeypatch.setattr(sampling, "grad_method", "hip")
    d, z, gy, gamma, beta, rm0, rv0 = _bn_inputs(name)
    vec = bb.facts(d["M"], d["N"])["vec"]
    # off the tape: stats + apply
    rm, rv = rm0.clone(), rv0.clone()
    mean, var, scale = dense.batch_norm_stats(z, gamma, bb.EPS, 0.1, rm, rv)
    want = dense.batch_norm_apply(z, mean, scale, beta, relu, l2)
    rm1, rv1 = rm0.clone(), rv0.clone()
    with torch.no_grad():
        off = dense.batch_norm(z, gamma, beta, bb.EPS, 0.1, rm1, rv1, relu=relu, l2norm=l2)
    assert torch.equal(off, want) and torch.equal(rm1, rm) and torch.equal(rv1, rv) and not off.requires_grad
    # on the tape: the same bits, the running statistics moved once
    runs = []
    for _ in range(2):
        zt, gt, bt = (t.clone().requires_grad_() for t in (z, gamma, beta))
        rm2, rv2 = rm0.clone(), rv0.clone()
        spy = _Spy(monkeypatch)
        y = dense.batch_norm(zt, gt, bt, bb.EPS, 0.1, rm2, rv2, relu=relu, l2norm=l2)
        assert spy.take() == ["ps_bn_batch_stats", "ps_bn_apply"]
        assert y.requires_grad and torch.equal(y, want) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
        y.backward(gy)
        assert spy.take() == ["ps_bn_bwd"]
        runs.append((zt.grad, gt.grad, bt.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # the gradients: the restatement's bits at the kernel's statistics, and the derived bound against float64 there
    stats = [_np(t) for t in (mean, var, scale)]
    e = bb.bn_bwd_exact(d["z"], d["gy"], *stats, d["beta"], bb.EPS, relu, l2, vec)
    got = dict(gz=_np(runs[0][0]), dgamma=_np(runs[0][1]), dbeta=_np(runs[0][2]))
    ref = bb.bn_bwd_64(d["z"], d["gy"], *stats, d["beta"], bb.EPS, relu, l2)
    bound = bb.bn_bwd_bound(d["z"], d["gy"], *stats, d["beta"], bb.EPS, relu, l2, vec)
    for k in OUT:
        assert bb.mismatches(got[k], e[k]) == [], k
        worst = float((np.abs(got[k] - ref[k]) / np.maximum(bound[k], 1e-300)).max())
        print(f"{name} {flags} {k}: max |got - ref64| / bound = {worst:.3f}")
        assert bb.outside(got[k], ref[k], bound[k]) == [], k
    # and against torch's autograd at the exact statistics, the fp32 statistics' own effect added (tests/test_bn_bwd_cases.py)
    m64, v64, s64 = bb.exact_stats_64(d["z"], d["gamma"], bb.EPS)
    at64 = bb.bn_bwd_64(d["z"], d["gy"], m64, v64, s64, d["beta"], bb.EPS, relu, l2)
    auto = bb.autograd_64(d["z"], d["gy"], d["gamma"], d["beta"], bb.EPS, relu, l2)
    for k in OUT:
        slack = np.abs(ref[k] - at64[k]) + 1e-9 * max(np.abs(auto[k]).max(), 1e-30)
        assert bb.outside(got[k], auto[k], bound[k] + slack) == [], k


def test_dense_batch_norm_routes(monkeypatch):
    from pinsage_hip import dense, sampling
    d, z, gy, gamma, beta, rm0, rv0 = _bn_inputs("vec4-2blocks")
    # grad_method "torch": no native call, torch's gradients
    monkeypatch.setattr(sampling, "grad_method", "torch")
    spy = _Spy(monkeypatch)
    zt, gt, bt = (t.clone().requires_grad_() for t in (z, gamma, beta))
    rm, rv = rm0.clone(), rv0.clone()
    y = dense.batch_norm(zt, gt, bt, bb.EPS, 0.1, rm, rv, relu=True, l2norm=True)
    y.backward(gy)
    assert not spy.take() and zt.grad is not None and not torch.equal(rm, rm0)
    # only what needs a gradient is computed
    monkeypatch.setattr(sampling, "grad_method", "hip")
    zt, gt, bt = z.clone().requires_grad_(), gamma.clone(), beta.clone()
    dense.batch_norm(zt, gt, bt, bb.EPS, 0.1, relu=True, l2norm=True).backward(gy)
    assert zt.grad is not None and gt.grad is None and bt.grad is None
    zt, gt, bt = z.clone(), gamma.clone().requires_grad_(), beta.clone()
    dense.batch_norm(zt, gt, bt, bb.EPS, 0.1, relu=True, l2norm=True).backward(gy)
    assert zt.grad is None and gt.grad is not None and bt.grad is None
    # float64 and CPU tensors: the torch expression
    spy.take()
    y = dense.batch_norm(z.double().requires_grad_(), gamma.double(), beta.double(), relu=True)
    assert y.dtype == torch.float64 and not spy.take()
    y = dense.batch_norm(z.cpu().requires_grad_(), gamma.cpu(), beta.cpu(), l2norm=True)
    assert not y.is_cuda and not spy.take()


# ---- GraphConvLayer, grad_method = "hip" -------------------------------------------------------------------------------------------
def _layer(prefix, cin, cout):
    from model import layers as L
    m = L.GraphConvLayer(cin, cout)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in lc.state_dict(prefix).items()}, strict=True)
    return m.cuda()


LAYERS = [("p_", 40, 48, "x_a", "n_a"), ("r_", 33, 21, "r_x", "r_n")]
LAYER_IDS = ["golden-40-48", "ragged-193x33-21"]


@pytest.mark.parametrize("prefix,cin,cout,kx,kn", LAYERS, ids=LAYER_IDS)
def test_graph_conv_layer_trains_on_the_kernels(prefix, cin, cout, kx, kn, monkeypatch):
    from pinsage_hip import sampling
    monkeypatch.setattr(sampling, "grad_method", "hip")
    g = lc.golden()
    x, n = _dev(g[kx]), _dev(g[kn])
    G = torch.randn(x.size(0), cout, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        ref = _layer(prefix, cin, cout).train()
        want = ref(x, n)
    spy = _Spy(monkeypatch)
    # a default layer under autograd: no native call
    m = _layer(prefix, cin, cout).train()
    out = m(x, n)
    assert not spy.take() and out.requires_grad
    steps = []
    for _ in range(2):
        m = _layer(prefix, cin, cout).train()
        m.grad_method = "hip"
        out = m(x, n)
        names = spy.take()
        assert "ps_bn_batch_stats" in names and "ps_bn_apply" in names and out.requires_grad
        assert torch.equal(out, want)
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(getattr(m.bn, k), getattr(ref.bn, k)), k
        (out * G).sum().backward()
        names = spy.take()
        assert "ps_bn_bwd" in names and "ps_linear_wgrad" in names
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        steps.append([p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*steps))


def test_graph_conv_layer_hip_dispatch(monkeypatch):
    from model import layers as L
    from pinsage_hip import sampling
    monkeypatch.setattr(sampling, "grad_method", "hip")
    g = lc.golden()
    x, n = _dev(g["x_a"]), _dev(g["n_a"])
    assert L.GraphConvLayer.grad_method == "torch"
    spy = _Spy(monkeypatch)
    # M == 1 is served on the tape in both modes, without batch norm and with the buffers untouched
    for mode in (True, False):
        m = _layer("p_", 40, 48).train(mode)
        m.grad_method = "hip"
        out = m(x[:1], n[:1])
        assert set(spy.take()) == {"ps_linear", "ps_bn_apply"} and out.requires_grad      # ps_bn_apply: LinearFn's row norm
        np.testing.assert_allclose(_np(out), g["out_m1"], rtol=lc.RTOL, atol=lc.ATOL)
        assert int(m.bn.num_batches_tracked) == 0 and not m.bn.running_mean.any()
        out.sum().backward()
        assert "ps_linear_wgrad" in spy.take() and m.linear_self.weight.grad is not None and m.bn.weight.grad is None
    # eval with gradients, M >= 2: torch
    m = _layer("p_", 40, 48).eval()
    m.grad_method = "hip"
    out = m(x, n)
    assert not spy.take() and out.requires_grad
    # an empty batch: torch
    m.train()
    assert m(x[:0], n[:0]).shape == (0, 48) and not spy.take()
    # sampling.grad_method "torch" switches every HIP backward off
    monkeypatch.setattr(sampling, "grad_method", "torch")
    assert m(x, n).requires_grad and not spy.take()
    monkeypatch.setattr(sampling, "grad_method", "hip")
    # a frozen batch-norm weight / bias is honoured
    m = _layer("p_", 40, 48).train()
    m.grad_method = "hip"
    m.bn.weight.requires_grad_(False)
    m.bn.bias.requires_grad_(False)
    m(x, n).square().sum().backward()
    assert "ps_bn_bwd" in spy.take()
    assert m.bn.weight.grad is None and m.bn.bias.grad is None and m.linear_out.weight.grad is not None
    # the class attribute is the switch as well
    monkeypatch.setattr(L.GraphConvLayer, "grad_method", "hip")
    m = _layer("p_", 40, 48).train()
    m(x, n)
    assert "ps_bn_batch_stats" in spy.take()


def _metrics(model, x, n, G, ref):
    """per tensor max |grad - ref64| / max |ref64| (the three linear biases: over ref's bias scale)"""
    model.zero_grad(set_to_none=True)
    xs, ns = x.clone().requires_grad_(), n.clone().requires_grad_()
    (model(xs, ns) * G).sum().backward()
    got = {k: p.grad for k, p in model.named_parameters()}
    got["x"], got["neigh_x"] = xs.grad, ns.grad
    out = {}
    for k, r in ref["grads"].items():
        scale = ref["bias_scale"] if k.startswith("linear") and k.endswith(".bias") else r.abs().max().item()
        out[k] = (got[k].double() - r).abs().max().item() / scale
    return out


@pytest.mark.parametrize("prefix,cin,cout,kx,kn", LAYERS, ids=LAYER_IDS)
def test_graph_conv_layer_gradients(prefix, cin, cout, kx, kn, monkeypatch):
    from pinsage_hip import sampling
    monkeypatch.setattr(sampling, "grad_method", "hip")
    g = lc.golden()
    x, n = _dev(g[kx]), _dev(g[kn])
    G = torch.randn(x.size(0), cout, generator=torch.Generator().manual_seed(6)).cuda()
    # float64 autograd of _forward_torch on a .double() copy, and dL/dz at the batch norm's input
    m64 = _layer(prefix, cin, cout).double().train()
    seen = []

    def keep_input(mod, inp, out):
        inp[0].retain_grad()
        seen.append(inp[0])
    m64.bn.register_forward_hook(keep_input)
    x64, n64 = x.double().requires_grad_(), n.double().requires_grad_()
    (m64._forward_torch(x64, n64) * G.double()).sum().backward()
    grads = {k: p.grad for k, p in m64.named_parameters()}
    grads["x"], grads["neigh_x"] = x64.grad, n64.grad
    ref = dict(grads=grads, bias_scale=seen[0].grad.abs().sum(dim=0).max().item())
    assert len(grads) == 10 and ref["bias_scale"] > 0
    torch_m = _layer(prefix, cin, cout).train()
    hip_m = _layer(prefix, cin, cout).train()
    hip_m.grad_method = "hip"
    spy = _Spy(monkeypatch)
    base = _metrics(torch_m, x, n, G, ref)
    assert not spy.take()
    got = _metrics(hip_m, x, n, G, ref)
    assert "ps_bn_bwd" in spy.take()
    for k in ref["grads"]:
        print(f"{prefix} {k:<22s} hip {got[k]:.3e}  torch fp32 {base[k]:.3e}  ratio {got[k] / base[k] if base[k] else float('inf'):.2f}")
    for k in ref["grads"]:
        assert got[k] <= 4.0 * base[k], (k, got[k], base[k])


def test_graph_conv_layer_tape_peak_memory(monkeypatch):
    """M = 16 384, 256 -> 256, a training forward on the tape: z and y (the backward keeps z, nothing else of [M, O]) -- at most
    2.5 [M, O] buffers plus the statistics workspace and the composed weights (Wo's halves, W1, W2 and the transposed copies)"""
    from model import layers as L
    from pinsage_hip import native as nv
    from pinsage_hip import sampling
    monkeypatch.setattr(sampling, "grad_method", "hip")
    M, C = 16384, 256
    torch.manual_seed(3)
    m = L.GraphConvLayer(C, C).cuda().train()
    m.grad_method = "hip"
    x, n = torch.randn(M, C, device="cuda"), torch.randn(M, C, device="cuda")
    m(x[:256], n[:256]).sum().backward()
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m(x, n)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    limit = int(2.5 * M * C * 4) + nv.lib().ps_bn_stats_workspace_bytes(M, C) + 8 * C * C * 4
    print(f"peak allocation above the inputs: {grew} bytes, limit {limit}, one [M, O] buffer {M * C * 4}")
    assert out.shape == (M, C) and out.requires_grad and grew <= limit
    out.sum().backward()
    assert m.bn.weight.grad is not None and torch.isfinite(m.linear_self.weight.grad).all()
