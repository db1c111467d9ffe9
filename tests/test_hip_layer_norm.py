"""ps_layer_norm and ps_layer_norm_bwd (csrc/layer_norm.hip) on the device against the exact restatements of
tests/helpers/ln_cases.py, bit for bit, over its case table and its live masks (the dead rows of x and gy hold NaN and Inf); the
aliasing, NULL-output and error contracts of include/pinsage_hip.h; dense.layer_norm on and off the autograd tape; and
model.aggregators.ImportanceAggregator with norm_method = "hip".

ImportanceAggregator's output and gradients are held to the torch module at rtol 1e-4 / atol 1e-5, the tolerance
tests/test_hip_model.py::test_aggregators_are_differentiable_wrt_features holds this module to."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import abi_cases as ac
from helpers import abi_cases_layer_norm  # noqa: F401  (the two entry points join ac.CASES)
from helpers import ln_cases as ln

pytestmark = pytest.mark.gpu
FWD, BWD = ("y", "mean", "rstd"), ("gx", "dgamma", "dbeta")
CANARY = 7.0


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


def _np(t):
    return t.detach().cpu().numpy()


def _new(*shape):
    return torch.full(shape, CANARY, dtype=torch.float32, device="cuda")


class _Call:
    """one case under one mask on the device: the inputs (dead rows poisoned), and the two entry points with fresh or given outputs"""

    def __init__(self, name, which="none", nan=False):
        from pinsage_hip import native as nv
        self.d = d = ln.data(name)
        self.off = ln.case(name)[3]
        self.M, self.N = d["M"], d["N"]
        self.live_np = ln.mask(which, self.M)
        x = ln.with_nan(d) if nan else d["x"]
        self.x = _dev(ln.poison(x, self.live_np), self.off)
        self.gy = _dev(ln.poison(d["gy"], self.live_np))
        self.gamma, self.beta = _dev(d["gamma"]), _dev(d["beta"])
        self.live = None if self.live_np is None else torch.tensor(np.array(self.live_np)).cuda()
        self.want = ln.expected(name, which, nan=nan)
        self.mean, self.rstd = _dev(self.want["mean"]), _dev(self.want["rstd"])
        self.wsb = nv.lib().ps_layer_norm_bwd_workspace_bytes(self.M, self.N)
        self.ws = torch.full((self.wsb,), 0xA5, dtype=torch.uint8, device="cuda")

    def fwd(self, y="new", mean="new", rstd="new", x="given", M=None, N=None, gamma="given", beta="given"):
        from pinsage_hip import native as nv
        y = _new(self.M, self.N) if isinstance(y, str) else y
        mean = _new(self.M) if isinstance(mean, str) else mean
        rstd = _new(self.M) if isinstance(rstd, str) else rstd
        pick = lambda v, own: own if isinstance(v, str) else v                       # noqa: E731
        rc = nv.lib().ps_layer_norm(nv.ptr(pick(x, self.x)), self.M if M is None else M, self.N if N is None else N,
                                    nv.ptr(pick(gamma, self.gamma)), nv.ptr(pick(beta, self.beta)), float(ln.EPS), nv.ptr(self.live),
                                    nv.ptr(y), nv.ptr(mean), nv.ptr(rstd), nv.stream())
        torch.cuda.synchronize()
        return rc, dict(y=y, mean=mean, rstd=rstd)

    def bwd(self, gx="new", dgamma="new", dbeta="new", gy="given", ws=None, wsb=None, M=None, N=None, **absent):
        from pinsage_hip import native as nv
        gx = _new(self.M, self.N) if isinstance(gx, str) else gx
        dgamma = _new(self.N) if isinstance(dgamma, str) else dgamma
        dbeta = _new(self.N) if isinstance(dbeta, str) else dbeta
        inp = dict(x=self.x, gy=self.gy if isinstance(gy, str) else gy, mean=self.mean, rstd=self.rstd, gamma=self.gamma)
        inp.update(absent)                                                           # x=None, ...: a NULL input
        rc = nv.lib().ps_layer_norm_bwd(nv.ptr(inp["x"]), nv.ptr(inp["gy"]), self.M if M is None else M, self.N if N is None else N,
                                        nv.ptr(inp["mean"]), nv.ptr(inp["rstd"]), nv.ptr(inp["gamma"]), nv.ptr(self.live), nv.ptr(gx),
                                        nv.ptr(dgamma), nv.ptr(dbeta), nv.ptr(self.ws) if ws is None else ws,
                                        self.wsb if wsb is None else wsb, nv.stream())
        torch.cuda.synchronize()
        return rc, dict(gx=gx, dgamma=dgamma, dbeta=dbeta)


def _same(got, want, keys, what):
    for k in keys:
        if got[k] is not None and want[k] is not None:
            w = want[k] if isinstance(want[k], np.ndarray) else _np(want[k])
            assert ln.mismatches(_np(got[k]), w) == [], (what, k)


# ---- the kernels against the restatements ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ln.MASKS)
@pytest.mark.parametrize("name", ln.NAMES)
def test_kernels_are_the_restatements(name, which):
    c = _Call(name, which)
    rc, got = c.fwd()
    assert rc == 0
    _same(got, c.want, FWD, (name, which))
    rc, back = c.bwd()
    assert rc == 0
    _same(back, c.want, BWD, (name, which))
    dead = ~ln.alive_rows(c.live_np, c.M)
    for k, t in (("y", got["y"]), ("gx", back["gx"]), ("mean", got["mean"]), ("rstd", got["rstd"])):
        a = _np(t)
        assert np.isfinite(a).all() and not a[dead].any() and not np.signbit(a[dead]).any(), k      # dead rows: +0.0
    assert np.isfinite(_np(back["dgamma"])).all() and np.isfinite(_np(back["dbeta"])).all()


@pytest.mark.parametrize("which", ["none", "first row dead"])
@pytest.mark.parametrize("name", ["vec1-partial", "vec1-2blocks", "vec4-2blocks", "v4-keep", "v4-keep+1", "v1-keep", "v1-keep+1", "long"])
def test_in_place_and_null_outputs(name, which):
    c = _Call(name, which)
    rc, fresh = c.fwd()
    assert rc == 0
    x = c.x.clone() if not c.off else _dev(_np(c.x), c.off)
    rc, alias = c.fwd(y=x, x=x)                                       # y = x
    assert rc == 0
    _same(alias, fresh, FWD, (name, "y = x"))
    rc, bare = c.fwd(mean=None, rstd=None)
    assert rc == 0
    _same(bare, fresh, ("y",), (name, "no statistics"))
    rc, back = c.bwd()
    assert rc == 0
    gy = c.gy.clone()
    rc, alias = c.bwd(gx=gy, gy=gy)                                   # gx = gy
    assert rc == 0
    _same(alias, back, BWD, (name, "gx = gy"))
    rc, part = c.bwd(gx=None)
    assert rc == 0
    _same(part, back, BWD, (name, "gx NULL"))
    rc, part = c.bwd(dgamma=None, dbeta=None, ws=ctypes.c_void_p(0), wsb=0)          # no workspace without the column sums
    assert rc == 0
    _same(part, back, BWD, (name, "dgamma / dbeta NULL"))
    before = c.ws.clone()
    rc, _ = c.bwd(gx=None, dgamma=None, dbeta=None)
    assert rc == 0 and torch.equal(c.ws, before)


def test_planted_rows():
    name = "vec4-2blocks"
    c = _Call(name)
    d, e = c.d, c.want
    _, got = c.fwd()
    _same(got, e, FWD, "planted")
    y = _np(got["y"])
    assert y[d["const_row"]].tobytes() == d["beta"].tobytes() and y[d["zero_row"]].tobytes() == d["beta"].tobytes()
    assert _np(got["rstd"])[d["const_row"]] == np.float32(1.0) / np.sqrt(np.float32(ln.EPS))
    ref = ln.ln_fwd_64(d["x"], d["gamma"], d["beta"], ln.EPS, None)
    assert abs(_np(got["rstd"])[d["hundred_row"]] / ref["rstd"][d["hundred_row"]] - 1) < 1e-4
    _, back = c.bwd()
    _same(back, e, BWD, "planted")
    # one NaN in a live row: that row is NaN, every dgamma is NaN, dbeta is finite, the other rows keep their bits
    n = _Call(name, nan=True)
    _, gn = n.fwd()
    _same(gn, n.want, FWD, "nan")
    _, bn = n.bwd()
    _same(bn, n.want, BWD, "nan")
    r = d["nan_row"]
    rest = torch.arange(d["M"], device="cuda") != r
    assert torch.isnan(gn["y"][r]).all() and torch.isnan(bn["gx"][r]).all()
    assert torch.isnan(bn["dgamma"]).all() and torch.isfinite(bn["dbeta"]).all()
    assert torch.equal(gn["y"][rest], got["y"][rest]) and torch.equal(bn["gx"][rest], back["gx"][rest])


def test_error_codes_leave_the_outputs_alone():
    from pinsage_hip import native as nv
    c = _Call("ragged-steps", "first row dead")
    keep = c.ws.clone()
    null = ctypes.c_void_p(0)

    def untouched(rc, out, code):
        assert rc == code, (rc, code)
        assert all((t == CANARY).all() for t in out.values() if t is not None)
        assert torch.equal(c.ws, keep)
    untouched(*c.fwd(M=-1), nv.PS_EINVAL)
    untouched(*c.fwd(N=0), nv.PS_EINVAL)
    untouched(*c.fwd(x=None), nv.PS_EINVAL)
    untouched(*c.fwd(gamma=None), nv.PS_EINVAL)
    untouched(*c.fwd(beta=None), nv.PS_EINVAL)
    untouched(*c.fwd(rstd=None), nv.PS_EINVAL)                        # one statistic alone
    untouched(*c.fwd(mean=None), nv.PS_EINVAL)
    assert c.fwd(y=None)[0] == nv.PS_EINVAL
    untouched(*c.fwd(M=0, x=None, gamma=None, beta=None), nv.PS_OK)   # no rows: whatever the pointers
    untouched(*c.bwd(M=-1), nv.PS_EINVAL)
    untouched(*c.bwd(N=0), nv.PS_EINVAL)
    for k in ("x", "gy", "mean", "rstd", "gamma"):
        untouched(*c.bwd(**{k: None}), nv.PS_EINVAL)
    untouched(*c.bwd(dgamma=None), nv.PS_EINVAL)                      # one of the pair alone
    untouched(*c.bwd(dbeta=None), nv.PS_EINVAL)
    untouched(*c.bwd(ws=null), nv.PS_EINVAL)
    untouched(*c.bwd(ws=ctypes.c_void_p(c.ws.data_ptr() + 4)), nv.PS_EINVAL)
    untouched(*c.bwd(wsb=c.wsb - 1), nv.PS_EWORKSPACE)
    fn = nv.lib().ps_layer_norm_bwd_workspace_bytes
    assert fn(0, 8) == 0 and fn(2, 0) == 0 and fn(129, 8) == 2 * 2 * 8 * 8
    # no rows: dgamma / dbeta are the sums of nothing, gx is not touched
    rc, out = c.bwd(M=0, x=None, gy=None, mean=None, rstd=None, gamma=None, ws=null, wsb=0)
    assert rc == nv.PS_OK and not out["dgamma"].any() and not out["dbeta"].any() and (out["gx"] == CANARY).all()


def test_more_column_blocks_than_a_grid_holds_is_unsupported():
    """N = 65 535 * 64 + 1, VEC 1: one column block more than grid.y takes.  PS_EUNSUPPORTED, and nothing is written."""
    from pinsage_hip import native as nv
    M, N = 2, 65535 * 64 + 1
    x, gy = (torch.zeros((M, N), dtype=torch.float32, device="cuda") for _ in range(2))
    gamma = torch.ones(N, dtype=torch.float32, device="cuda")
    mean, rstd = (torch.ones(M, dtype=torch.float32, device="cuda") for _ in range(2))
    out = [_new(*s) for s in ((M, N), (N,), (N,))]
    wsb = nv.lib().ps_layer_norm_bwd_workspace_bytes(M, N)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = nv.lib().ps_layer_norm_bwd(nv.ptr(x), nv.ptr(gy), M, N, nv.ptr(mean), nv.ptr(rstd), nv.ptr(gamma), nv.ptr(None),
                                    *(nv.ptr(o) for o in out), nv.ptr(ws), wsb, nv.stream())
    torch.cuda.synchronize()
    assert rc == nv.PS_EUNSUPPORTED
    assert all((o == CANARY).all() for o in out) and (ws == 0xFF).all()


@pytest.mark.parametrize("name", ["ps_layer_norm", "ps_layer_norm_bwd"])
def test_contract_matrix_holds_the_layer_norm(name):
    """The contract matrix of tests/test_hip_abi_contract.py (captured stream, poisoned outputs and workspace, guard bands, replays)
    for the two entry points, started from here as well: that module parametrises over the case table when it is collected, and a
    run of it alone does not import the case module of these entry points."""
    import test_hip_abi_contract as contract
    assert name in ac.CASES
    contract.test_contract(name)


# ---- dense.layer_norm ------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("which", ["none", "last row of a partition dead"])
@pytest.mark.parametrize("name", ["ragged-steps", "vec1-2blocks", "vec4-2blocks"])
def test_dense_layer_norm(name, which, monkeypatch):
    from pinsage_hip import dense, sampling
    monkeypatch.setattr(sampling, "grad_method", "hip")
    c = _Call(name, which)
    e = c.want
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        off = dense.layer_norm(c.x, c.gamma, c.beta, ln.EPS, c.live)
    assert spy.take() == ["ps_layer_norm"] and not off.requires_grad
    assert ln.mismatches(_np(off), e["y"]) == []
    y, mean, rstd = dense.layer_norm_fwd(c.x, c.gamma, c.beta, ln.EPS, c.live)
    _same(dict(y=y, mean=mean, rstd=rstd), e, FWD, "layer_norm_fwd")
    runs = []
    for _ in range(2):
        xt, gt, bt = (t.clone().requires_grad_() for t in (c.x, c.gamma, c.beta))
        spy.take()
        y = dense.layer_norm(xt, gt, bt, ln.EPS, c.live)
        assert spy.take() == ["ps_layer_norm"] and y.requires_grad and torch.equal(y, off)
        y.backward(c.gy)
        assert spy.take() == ["ps_layer_norm_bwd"]
        runs.append(dict(gx=xt.grad, dgamma=gt.grad, dbeta=bt.grad))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in BWD)
    _same(runs[0], e, BWD, "LayerNormFn")


def test_dense_layer_norm_routes(monkeypatch):
    from pinsage_hip import dense, sampling
    c = _Call("vec4-2blocks", "first row dead")
    d = ln.data("vec4-2blocks")
    x, gy = _dev(d["x"]), _dev(d["gy"])                               # no poison: torch reads every row
    # grad_method "torch": no native call, torch's gradients
    monkeypatch.setattr(sampling, "grad_method", "torch")
    spy = _Spy(monkeypatch)
    xt, gt, bt = (t.clone().requires_grad_() for t in (x, c.gamma, c.beta))
    y = dense.layer_norm(xt, gt, bt, ln.EPS, c.live)
    y.backward(gy)
    assert not spy.take() and xt.grad is not None and not y[0].any() and not xt.grad[0].any()
    ref = torch.where((c.live > 0)[:, None], F.layer_norm(x, (d["N"],), c.gamma, c.beta, ln.EPS), torch.zeros_like(x))
    assert torch.equal(y, ref)
    # only what needs a gradient is computed
    monkeypatch.setattr(sampling, "grad_method", "hip")
    xt, gt, bt = x.clone().requires_grad_(), c.gamma.clone(), c.beta.clone()
    dense.layer_norm(xt, gt, bt, ln.EPS, c.live).backward(gy)
    assert xt.grad is not None and gt.grad is None and bt.grad is None
    xt, gt, bt = x.clone(), c.gamma.clone().requires_grad_(), c.beta.clone()
    dense.layer_norm(xt, gt, bt, ln.EPS, c.live).backward(gy)
    assert xt.grad is None and gt.grad is not None and bt.grad is None
    assert spy.take() == ["ps_layer_norm", "ps_layer_norm_bwd"] * 2
    # float64 and CPU tensors: the torch expression
    y = dense.layer_norm(x.double().requires_grad_(), c.gamma.double(), c.beta.double(), ln.EPS, c.live)
    assert y.dtype == torch.float64 and not spy.take()
    y = dense.layer_norm(x.cpu().requires_grad_(), c.gamma.cpu(), c.beta.cpu(), ln.EPS, c.live.cpu())
    assert not y.is_cuda and not spy.take()


# ---- ImportanceAggregator, norm_method = "hip" ------------------------------------------------------------------------------------
def _lists():
    """the 50-node neighbour and weight lists of tests/test_hip_model.py::test_aggregators_are_differentiable_wrt_features (some empty)"""
    rs = np.random.RandomState(8)
    nb = [[int(v) for v in rs.randint(0, 50, size=i % 6)] for i in range(50)]
    wt = [[float(v) for v in rs.random_sample(i % 6) + 0.05] for i in range(50)]
    return nb, wt


def _aggregator(method):
    from model.aggregators import ImportanceAggregator
    torch.manual_seed(4)
    m = ImportanceAggregator(24, 12)
    with torch.no_grad():
        m.norm.weight.copy_(torch.linspace(0.5, 1.5, 12))
        m.norm.bias.copy_(torch.linspace(-0.3, 0.3, 12))
    m.norm_method = method
    return m.cuda()


def _step(m, x0, nb, wt, G):
    m.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_()
    out = m(x, nb, wt)
    (out * G).sum().backward()
    return [out.detach(), x.grad] + [p.grad for p in m.parameters()]


def test_importance_aggregator_trains_on_the_kernels(monkeypatch):
    from pinsage_hip import sampling
    monkeypatch.setattr(sampling, "grad_method", "hip")
    nb, wt = _lists()
    empty = torch.tensor([len(a) == 0 for a in nb], device="cuda")
    assert empty.any() and not empty.all()
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(50, 24, generator=g).cuda()
    G = torch.randn(50, 12, generator=g).cuda()
    spy = _Spy(monkeypatch)

    def no_torch(*a, **k):
        raise AssertionError("the kernel path reached F.layer_norm / F.linear")
    want = _step(_aggregator("torch"), x0, nb, wt, G)
    assert "ps_layer_norm" not in spy.take()
    runs = []
    for _ in range(2):
        m = _aggregator("hip")
        with monkeypatch.context() as mp:
            mp.setattr(F, "layer_norm", no_torch)
            mp.setattr(F, "linear", no_torch)
            m.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_()
            out = m(x, nb, wt)
            assert spy.take() == ["ps_importance_pool", "ps_linear", "ps_layer_norm"] and out.requires_grad
            (out * G).sum().backward()
            back = spy.take()
            # the three backwards; LinearFn's input gradient is ps_linear over W^T, PoolFn restates its weights with ps_pool_weights
            need = {"ps_layer_norm_bwd", "ps_linear_wgrad", "ps_gather_bwd"}
            assert need <= set(back) <= need | {"ps_linear", "ps_pool_weights"}, back
            assert back[0] == "ps_layer_norm_bwd" and back[-1] == "ps_gather_bwd"
            with torch.no_grad():
                off = m(x0, nb, wt)
            assert spy.take() == ["ps_importance_pool", "ps_linear", "ps_layer_norm"] and torch.equal(off, out)
        runs.append([out.detach(), x.grad] + [p.grad for p in m.parameters()])
    assert len(want) == 6 and all(t is not None for t in runs[0])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                      # the same bits on every run
    for got, ref in zip(runs[0], want):
        np.testing.assert_allclose(_np(got), _np(ref), rtol=1e-4, atol=1e-5)
    out, gx = runs[0][0], runs[0][1]
    assert not out[empty].any() and not torch.signbit(out[empty]).any()               # empty rows: exact zeros
    # ... with zero gradient: what arrives at an empty row reaches no gradient (the same bits with it tripled), and a node that no
    # list names gets none
    G3 = G.clone()
    G3[empty] *= 3.0
    for a, b in zip(_step(_aggregator("hip"), x0, nb, wt, G3), runs[0]):
        assert torch.equal(a, b)
    named = torch.zeros(50, dtype=torch.bool)
    named[[v for a in nb for v in a]] = True
    assert not gx[~named.cuda()].any()
    # sampling.grad_method "torch": the same python, dense.* fall back by themselves
    monkeypatch.setattr(sampling, "grad_method", "torch")
    spy.take()
    tor = _step(_aggregator("hip"), x0, nb, wt, G)
    names = spy.take()
    assert "ps_layer_norm" not in names and "ps_layer_norm_bwd" not in names and "ps_linear_wgrad" not in names
    for got, ref in zip(tor, want):
        np.testing.assert_allclose(_np(got), _np(ref), rtol=1e-4, atol=1e-5)


def test_importance_aggregator_default_keeps_its_bits_and_cpu_tensors_their_code(monkeypatch):
    from pinsage_hip import sampling
    monkeypatch.setattr(sampling, "grad_method", "hip")
    nb, wt = _lists()
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(50, 24, generator=g).cuda()
    m = _aggregator("torch")
    # the default's forward, restated as the module computed it before the switch existed
    x = x0.clone().requires_grad_()
    out = m(x, nb, wt)
    x2 = x0.clone().requires_grad_()
    from model import aggregators as A
    pooled = A._pool(x2, *A._pad(nb, 50, wt))
    t = F.linear(pooled, m.transform.weight, m.transform.bias)
    normed = F.layer_norm(t, m.norm.normalized_shape, m.norm.weight, m.norm.bias, m.norm.eps)
    has = torch.tensor([len(a) > 0 for a in nb], device="cuda")[:, None]
    assert torch.equal(out, torch.where(has, normed, torch.zeros_like(normed)))
    # CPU tensors: "hip" and "torch" run the same code: identical bits for the output and all gradients
    G = torch.randn(50, 12, generator=g)
    steps = []
    for method in ("torch", "hip"):
        mc = _aggregator(method).cpu()
        spy = _Spy(monkeypatch)
        steps.append(_step(mc, x0.cpu(), nb, wt, G))
        assert "ps_layer_norm" not in spy.take()
    assert all(torch.equal(a, b) for a, b in zip(*steps))
    # a norm that is not exactly nn.LayerNorm keeps the torch code under "hip"
    class OtherNorm(torch.nn.LayerNorm):
        pass
    mh = _aggregator("hip")
    mh.norm = OtherNorm(12).cuda()
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        other = mh(x0, nb, wt)
    assert "ps_layer_norm" not in spy.take() and other.shape == (50, 12)
