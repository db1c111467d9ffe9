"""The exact SpMM, its backward and the GraphConv edge branch that trains on them (csrc/spmm_exact.hip, pinsage_hip/graph.py) on
the GPU:

  1. ps_spmm_csr_exact over the target and over the source CSR, and ps_sddmm_csr, equal the numpy restatement of
     tests/helpers/spmm_cases.py bit for bit, and themselves on a second run;
  2. empty problems and argument errors;
  3. graph.spmm against the torch formulation on the same leaves, with every combination of which leaf needs a gradient;
  4. GraphConv and the PinSage edge branch: the same bits twice, the torch method within the gradient tolerance, and which entry
     points each method calls;
  5. a training step allocates no [E, H] tensor.

Outputs are filled with NaN and workspaces with 0xff before every raw call."""
import itertools

import numpy as np
import pytest
import torch

from helpers import spmm_cases as sc

pytestmark = pytest.mark.gpu
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-5           # the project's gradient tolerance (tests/test_hip_agg_bwd.py)
NEW = {"ps_spmm_csr_exact", "ps_sddmm_csr"}
NAMES = sc.names()


def _dev(a, offset=0):
    """a on the device; offset: that many elements into its storage (contiguous, not 16-byte aligned for one float)"""
    a = np.ascontiguousarray(a)
    if not offset:
        t = torch.tensor(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + offset, dtype=torch.tensor(a[:0]).dtype, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.tensor(a))
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t


def _nan(shape, offset=0):
    n = int(np.prod(shape))
    buf = torch.full((n + offset,), float("nan"), dtype=torch.float32, device="cuda")
    return buf[offset:].view(shape)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(np.argwhere(bad)[0])}"


def _close(a, b, what):
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=what)


def _raw_spmm(rowptr, col, val, x, V, offset=0):
    from pinsage_hip import native as nv
    N, H = x.shape
    E = col.numel()
    out = _nan((V, H), offset)
    n = nv.lib().ps_spmm_csr_exact_workspace_bytes(E, H)
    ws = torch.full((max(n, 1),), 0xff, dtype=torch.uint8, device="cuda")
    nv.call("ps_spmm_csr_exact", nv.ptr(rowptr), nv.ptr(col), nv.ptr(val), nv.ptr(x), N, H, V, E, nv.ptr(out), nv.ptr(ws), n,
            nv.stream())
    return out


def _raw_sddmm(rowptr, col, x, g):
    from pinsage_hip import native as nv
    N, H = x.shape
    d = _nan((col.numel(),))
    nv.call("ps_sddmm_csr", nv.ptr(rowptr), nv.ptr(col), nv.ptr(x), N, nv.ptr(g), g.shape[0], H, col.numel(), nv.ptr(d), nv.stream())
    return d


# ---- 1: bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_kernels_bit_exact(name):
    c, want = sc.case(name), sc.expected(name)
    o, V = c["offset"], c["V"]
    x, g = _dev(c["x"], o), _dev(c["g"], o)
    rowptr, col = _dev(c["rowptr"]), _dev(c["col"])
    val = None if c["val"] is None else _dev(c["val"])
    out = _raw_spmm(rowptr, col, val, x, V, o)
    _same(out, want["out"], f"{name}: out")
    _same(_raw_spmm(rowptr, col, val, x, V, o), out, f"{name}: out, second run")
    assert not _bits(out)[np.diff(c["rowptr"]) == 0].any()       # +0.0 in the empty rows
    s_rowptr, s_col = _dev(c["s_rowptr"]), _dev(c["s_col"])
    s_val = None if c["s_val"] is None else _dev(c["s_val"])
    dx = _raw_spmm(s_rowptr, s_col, s_val, g, V, o)
    _same(dx, want["dx"], f"{name}: dx over the source CSR")
    _same(_raw_spmm(s_rowptr, s_col, s_val, g, V, o), dx, f"{name}: dx, second run")
    d = _raw_sddmm(rowptr, col, x, g)
    _same(d, want["dval"], f"{name}: dval")
    _same(_raw_sddmm(rowptr, col, x, g), d, f"{name}: dval, second run")


def test_source_csr_is_the_transposition():
    """TargetCSR.source(): the same edges grouped by source with ps_csr_build's stable sort, and the index that carries val"""
    from pinsage_hip import graph as G
    rs = np.random.RandomState(3)
    V, E = 40, 700
    ei = torch.tensor(rs.randint(0, V, size=(2, E)), dtype=torch.int64, device="cuda")
    tc = G.TargetCSR(ei, V)
    s, index = tc.source()
    assert tc.source()[0] is s                                    # built once
    src, dst = ei[0].cpu().numpy(), ei[1].cpu().numpy()
    order = np.argsort(src, kind="stable")
    assert np.array_equal(s.perm.cpu().numpy(), order) and np.array_equal(s.col.cpu().numpy(), dst[order])
    assert np.array_equal(s.rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]))
    w = torch.tensor(rs.random_sample(E).astype(np.float32), device="cuda")
    assert torch.equal(w[tc.perm][index], w[s.perm])              # target-slot order -> source-slot order: one gather
    assert index.dtype == torch.int64 and (s.V, s.E) == (V, E)


# ---- 2: empty problems and argument errors -----------------------------------------------------------------------------------
def test_empty_problems_and_argument_errors():
    from pinsage_hip import native as nv
    lib = nv.lib()
    c = sc.case("straddle")
    V, N, H, E = c["V"], c["N"], c["H"], c["E"]
    rowptr, col, val, x, g = (_dev(c[k]) for k in ("rowptr", "col", "val", "x", "g"))
    out, d = _nan((V, H)), _nan((E,))
    n = lib.ps_spmm_csr_exact_workspace_bytes(E, H)
    assert n > 0 and lib.ps_spmm_csr_exact_workspace_bytes(0, H) == 0 and lib.ps_spmm_csr_exact_workspace_bytes(E, 0) == 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    p, st, null = nv.ptr, nv.stream(), nv.ptr(None)
    OK, EINVAL = nv.PS_OK, nv.PS_EINVAL
    assert lib.ps_spmm_exact_slice() == sc.slice_len() > 0
    # empty problems, whatever the pointers
    assert lib.ps_spmm_csr_exact(null, null, null, null, 0, H, 0, 0, null, null, 0, st) == OK
    assert lib.ps_spmm_csr_exact(null, null, null, null, 5, H, 0, 7, null, null, 0, st) == OK
    assert lib.ps_sddmm_csr(null, null, null, 0, null, 0, H, 0, null, st) == OK
    assert lib.ps_sddmm_csr(null, null, null, N, null, V, H, 0, null, st) == OK
    assert lib.ps_spmm_csr_exact(null, null, null, null, N, H, V, 0, p(out), null, 0, st) == OK      # E == 0: out zeroed
    torch.cuda.synchronize()
    assert not _bits(out).any()
    out.fill_(float("nan"))
    # refused calls
    args = dict(rowptr=p(rowptr), col=p(col), val=p(val), x=p(x), N=N, H=H, V=V, E=E, out=p(out), ws=p(ws), n=n)

    def spmm(**kw):
        a = dict(args, **kw)
        return lib.ps_spmm_csr_exact(a["rowptr"], a["col"], a["val"], a["x"], a["N"], a["H"], a["V"], a["E"], a["out"], a["ws"],
                                     a["n"], st)
    for kw in (dict(rowptr=null), dict(col=null), dict(x=null), dict(out=null), dict(ws=null), dict(H=0), dict(H=-4), dict(E=-1),
               dict(V=-1), dict(N=-1), dict(n=n - 1)):
        assert spmm(**kw) == EINVAL, kw
    assert spmm(E=1 << 41, n=1 << 62) == nv.PS_EUNSUPPORTED         # more slices than a grid holds: refused before any launch
    sargs = dict(rowptr=p(rowptr), col=p(col), x=p(x), N=N, g=p(g), V=V, H=H, E=E, d=p(d))

    def sddmm(**kw):
        a = dict(sargs, **kw)
        return lib.ps_sddmm_csr(a["rowptr"], a["col"], a["x"], a["N"], a["g"], a["V"], a["H"], a["E"], a["d"], st)
    for kw in (dict(rowptr=null), dict(col=null), dict(x=null), dict(g=null), dict(d=null), dict(H=0), dict(E=-1), dict(V=-1),
               dict(N=-1)):
        assert sddmm(**kw) == EINVAL, kw
    assert sddmm(E=1 << 41) == nv.PS_EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(d).all()       # a refused call writes nothing
    assert spmm(val=null) == OK and sddmm() == OK
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(d).any()


# ---- 3: graph.spmm against the torch formulation -------------------------------------------------------------------------------
def _hub_graph(V=300, seed=5):
    """about 300 nodes; node V // 2 receives (and sends) 2 S + 40 edges, so its row crosses two slice boundaries in both CSRs"""
    S = sc.slice_len()
    rs = np.random.RandomState(seed)
    hub = V // 2
    others = rs.randint(0, V, size=(2, 600))
    spokes = rs.randint(0, V, size=2 * S + 40)
    src = np.concatenate([others[0], spokes, np.full_like(spokes, hub)])
    dst = np.concatenate([others[1], np.full_like(spokes, hub), spokes])
    order = rs.permutation(src.size)
    return torch.tensor(np.stack([src[order], dst[order]]), dtype=torch.int64, device="cuda"), hub


def _grads(fn, leaves, need, g):
    ls = [t.detach().clone().requires_grad_(n) for t, n in zip(leaves, need)]
    out = fn(*ls)
    if g is None:
        out.sum().backward()                                      # hands the backward a stride-0 gradient
    else:
        out.backward(g)
    return out.detach(), [t.grad for t in ls]


@pytest.mark.parametrize("H", (8, 10))
def test_spmm_function_against_torch(H):
    """positive features, weights and gradients: no sum cancels, so the tolerance is a relative one everywhere"""
    from pinsage_hip import graph as G
    from pinsage_hip import sampling
    assert sampling.grad_method == "hip"
    S = sc.slice_len()
    ei, hub = _hub_graph()
    V = 300
    tc = G.TargetCSR(ei, V)
    for csr in (tc, tc.source()[0]):
        lo, hi = (int(v) for v in csr.rowptr[hub:hub + 2])
        assert (hi - 1) // S - lo // S >= 2                       # the hub is cut twice
    rs = np.random.RandomState(17)
    x = torch.tensor(rs.random_sample((V, H)).astype(np.float32) + 0.5, device="cuda")
    w = torch.tensor(rs.random_sample(tc.E).astype(np.float32) + 0.05, device="cuda")
    g = torch.tensor(rs.random_sample((V, H)).astype(np.float32) + 0.5, device="cuda")
    src, dst = ei[0], ei[1]

    def hip(xx, ww):
        return G.spmm(tc, xx, ww[tc.perm])

    def ref(xx, ww):
        return torch.zeros_like(xx).index_add_(0, dst, xx[src] * ww.view(-1, 1))
    for need in itertools.product((False, True), repeat=2):
        if not any(need):
            _close(hip(x, w), ref(x, w), "out, nothing on the tape")
            continue
        for gg in (g, None):
            o1, g1 = _grads(hip, [x, w], need, gg)
            o2, g2 = _grads(ref, [x, w], need, gg)
            _close(o1, o2, f"out with {need}")
            for name, n, a, b in zip(("x", "w"), need, g1, g2):
                if not n:
                    assert a is None, f"{name} is frozen and received a gradient"
                else:
                    _close(a, b, f"d{name} with {need}")
    # without edge values
    o1, (g1,) = _grads(lambda xx: G.spmm(tc, xx), [x], [True], g)
    o2, (g2,) = _grads(lambda xx: torch.zeros_like(xx).index_add_(0, dst, xx[src]), [x], [True], g)
    _close(o1, o2, "out, val None")
    _close(g1, g2, "dx, val None")
    # a recorded backward keeps the differentiable torch code: a gradient of a gradient
    def second(fn):
        xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        gx, = torch.autograd.grad(fn(xx, ww).square().sum(), xx, create_graph=True)
        gx.square().sum().backward()
        return ww.grad
    _close(second(hip), second(ref), "dw of a recorded backward")


# ---- 4: GraphConv and the PinSage edge branch ------------------------------------------------------------------------------------
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
        return set(names)


def _step(module, args, leaves, need, spy):
    """(out, leaf grads, parameter grads, names called in forward, names called in backward) of one forward + backward.  The
    modules end in F.normalize, so sum(out^2) is a constant whose gradient is zero (two methods would be compared on their
    rounding noise): the backward starts from a fixed random gradient of out instead."""
    module.zero_grad(set_to_none=True)
    ls = [t.detach().clone().requires_grad_(n) for t, n in zip(leaves, need)]
    spy.take()
    out = module(*args(ls))
    fwd = spy.take()
    out.backward(torch.tensor(np.random.RandomState(41).standard_normal(tuple(out.shape)).astype(np.float32), device="cuda"))
    bwd = spy.take()
    return out.detach(), [t.grad for t in ls], [p.grad.clone() for p in module.parameters()], fwd, bwd


@pytest.mark.parametrize("C,weights", [(8, "none"), (8, "both-grad"), (10, "edge-frozen"), (10, "importance-grad")])
def test_graphconv_trains_on_hip(C, weights, monkeypatch):
    from model.pinsage import GraphConv
    from pinsage_hip import sampling
    assert sampling.grad_method == "hip"
    ei, _ = _hub_graph()
    V, E = 300, ei.size(1)
    rs = np.random.RandomState(23)
    torch.manual_seed(C)
    conv = GraphConv(C, C).cuda()
    x = torch.tensor(rs.random_sample((V, C)).astype(np.float32) + 0.5, device="cuda")
    ew = torch.tensor(rs.random_sample(E).astype(np.float32) + 0.05, device="cuda")
    iw = torch.tensor(rs.random_sample(E).astype(np.float32) + 0.05, device="cuda")
    leaves, need, args = {
        "none": ([x], [True], lambda ls: (ls[0], ei)),
        "both-grad": ([x, ew, iw], [True, True, True], lambda ls: (ls[0], ei, ls[1], ls[2])),
        "edge-frozen": ([x, ew], [True, False], lambda ls: (ls[0], ei, ls[1])),
        "importance-grad": ([x, iw], [False, True], lambda ls: (ls[0], ei, None, ls[1])),
    }[weights]
    spy = _Spy(monkeypatch)
    a = _step(conv, args, leaves, need, spy)
    b = _step(conv, args, leaves, need, spy)
    for run in (a, b):
        assert "ps_spmm_csr_exact" in run[3] and "ps_spmm_csr_exact" in run[4] and "ps_spmm_csr" not in run[3] | run[4]
        assert "ps_sddmm_csr" not in run[3]
        assert ("ps_sddmm_csr" in run[4]) == (weights in ("both-grad", "importance-grad"))
    for p, q in zip([a[0]] + a[1] + a[2], [b[0]] + b[1] + b[2]):
        assert (p is None) == (q is None)
        if p is not None:
            _same(p, q, f"{weights}: two passes")
    monkeypatch.setattr(sampling, "grad_method", "torch")
    r = _step(conv, args, leaves, need, spy)
    monkeypatch.setattr(sampling, "grad_method", "hip")
    assert not (r[3] | r[4]) & (NEW | {"ps_spmm_csr"})
    _close(a[0], r[0], f"{weights} out")
    for n, p, q in zip(need, a[1], r[1]):
        assert (p is not None) == n == (q is not None)
        if n:
            _close(p, q, f"{weights} leaf gradients")
    for p, q in zip(a[2], r[2]):
        _close(p, q, f"{weights} parameter gradients")
    # inference keeps the atomic kernel
    spy.take()
    with torch.no_grad():
        o = conv(*args(leaves))
    called = spy.take()
    assert "ps_spmm_csr" in called and not called & NEW
    _close(o, a[0], f"{weights}: no_grad forward")


def test_pinsage_edge_branch_trains_on_hip(monkeypatch):
    from model.pinsage import PinSage
    from pinsage_hip import sampling
    ei, _ = _hub_graph()
    rs = np.random.RandomState(29)
    torch.manual_seed(2)
    model = PinSage(16, 32, 8, 2).cuda()
    x = torch.tensor(rs.random_sample((300, 16)).astype(np.float32) + 0.5, device="cuda")
    spy = _Spy(monkeypatch)

    def args(ls):
        return (ls[0],)

    class Edge(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = model

        def forward(self, xx):
            return self.m(xx, edge_index=ei)
    net = Edge()
    a = _step(net, args, [x], [True], spy)
    b = _step(net, args, [x], [True], spy)
    assert "ps_spmm_csr_exact" in a[3] and "ps_spmm_csr_exact" in a[4] and "ps_sddmm_csr" not in a[3] | a[4]
    for p, q in zip([a[0]] + a[1] + a[2], [b[0]] + b[1] + b[2]):
        _same(p, q, "PinSage edge branch: two passes")
    monkeypatch.setattr(sampling, "grad_method", "torch")
    r = _step(net, args, [x], [True], spy)
    monkeypatch.setattr(sampling, "grad_method", "hip")
    assert not (r[3] | r[4]) & NEW
    for p, q in zip([a[0]] + a[1] + a[2], [r[0]] + r[1] + r[2]):
        _close(p, q, "PinSage edge branch against the torch method")
    spy.take()
    with torch.no_grad():
        o = model(x, edge_index=ei)
    called = spy.take()
    assert "ps_spmm_csr" in called and not called & NEW
    _close(o, a[0], "PinSage edge branch: no_grad forward")


# ---- 5: peak allocation ----------------------------------------------------------------------------------------------------------
def test_training_step_builds_no_edge_by_feature_tensor(monkeypatch):
    """V = 256, E = 100 000, H = 64, one GraphConv forward + backward with an edge weight that needs a gradient: the peak rises by
    less than a quarter of ONE [E, H] fp32 tensor (E H bytes) with the HIP method -- its own tensors are a few [V, H] and [E]
    vectors and the index temporaries of torch's w[perm] backward --; the torch method builds at least two such tensors"""
    from model.pinsage import GraphConv
    from pinsage_hip import sampling
    V, E, H = 256, 100_000, 64
    rs = np.random.RandomState(31)
    ei = torch.tensor(rs.randint(0, V, size=(2, E)), dtype=torch.int64, device="cuda")
    x = torch.tensor(rs.random_sample((V, H)).astype(np.float32) + 0.5, device="cuda")
    ew = torch.tensor(rs.random_sample(E).astype(np.float32) + 0.05, device="cuda")
    torch.manual_seed(7)
    conv = GraphConv(H, H).cuda()

    def peak():
        conv.zero_grad(set_to_none=True)
        xx, ww = x.clone().requires_grad_(True), ew.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        conv(xx, ei, ww).square().sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, xx.grad, ww.grad
    peak()                                                        # warm-up: builds and caches both CSRs
    grew, gx, gw = peak()
    monkeypatch.setattr(sampling, "grad_method", "torch")
    grew_torch, gx_torch, gw_torch = peak()
    print(f"peak allocation: HIP method {grew} bytes, torch method {grew_torch} bytes; one [E,H] fp32 tensor {4 * E * H}")
    assert grew < E * H
    assert grew_torch >= 2 * 4 * E * H
    _close(gx, gx_torch, "dx at the large shape")
    _close(gw, gw_torch, "dw at the large shape")
