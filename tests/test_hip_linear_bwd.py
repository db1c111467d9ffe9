"""The backward of the dense layers on the GPU (csrc/linear_bwd.hip, pinsage_hip/dense.py: LinearFn, model/pinsage.py):

  1. ps_linear_wgrad equals linear_bwd_cases.wgrad_exact / bias_grad_exact bit for bit, and itself on a second run: every row
     count around the partition size P (read from the library), every (N, K) of the table, operands 4 bytes off a 16-byte
     boundary (the 4-byte sweeps: the same bits), db NULL, M = 0, the first M whose partition is 2 P, the error codes;
  2. ps_linear_epilogue_bwd equals epilogue_bwd_exact: every N of the table, the four flag sets, 4 bytes off, in place, the
     planted zero / near-clamp rows, a NaN in t;
  3. dense.linear on the tape: a grad_fn, gradients exactly for the leaves that need one, within linear_bwd_cases'
     layer_grad_bounds of torch float64 autograd and of grad_method = "torch", the same bits twice, and the entry points called;
  4. one training step of the three PinSage branches, and what no_grad inference runs.

Outputs are filled with NaN and workspaces with 0xff before every raw call.  Bounds: tests/helpers/linear_bwd_cases.py."""
import itertools

import numpy as np
import pytest
import torch

from helpers import gemm_cases as gc
from helpers import linear_bwd_cases as lb

pytestmark = pytest.mark.gpu
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-5           # the project's gradient tolerance (tests/test_hip_agg_bwd.py)
NEW = {"ps_linear_wgrad", "ps_linear_epilogue_bwd"}
PS_EINVAL, PS_EWORKSPACE = -1, -3
ROW_NAMES = ("1", "2", "3", "P-1", "P", "P+1", "2P+3")


def _rows(name):
    P = lb.partition(1)
    return dict(zip(ROW_NAMES, lb.wgrad_rows(P)))[name]


def _dev(a, offset=0):
    """a on the device; offset: that many elements into its storage (contiguous, not 16-byte aligned for one float)"""
    a = np.ascontiguousarray(a)
    if not offset:
        t = torch.tensor(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.tensor(a))
    assert t.is_contiguous() and (a.size == 0 or t.data_ptr() % 16 != 0)
    return t


def _nan(shape, offset=0):
    n = int(np.prod(shape))
    buf = torch.full((n + offset,), float("nan"), dtype=torch.float32, device="cuda")
    return buf[offset:].view(shape)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


def _same(got, want, what):
    got = _host(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float32)
    want = _host(want) if isinstance(want, torch.Tensor) else np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = lb.mismatches(got, want)
    assert bad == [], f"{what}: first differences (row, col, got, want) {bad}"


def _wgrad(g, x, bias=True, offset=0, ws_fill=0xff):
    """raw ps_linear_wgrad -> (status, dW, db)"""
    from pinsage_hip import native as nv
    M, N = g.shape
    K = x.shape[1]
    dW, db = _nan((N, K), offset), (_nan((N,), offset) if bias else None)
    n = nv.lib().ps_linear_wgrad_workspace_bytes(M, N, K)
    ws = torch.full((max(n, 1),), ws_fill, dtype=torch.uint8, device="cuda")
    rc = nv.lib().ps_linear_wgrad(nv.ptr(g), M, N, nv.ptr(x), K, nv.ptr(dW), nv.ptr(db), nv.ptr(ws) if n else None, n, nv.stream())
    return rc, dW, db


# ---- 1: ps_linear_wgrad ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROW_NAMES)
@pytest.mark.parametrize("N,K", lb.WGRAD_SHAPES)
def test_wgrad_equals_the_restatement(N, K, rows):
    M = _rows(rows)
    P = lb.partition(M)
    g, x = lb.wgrad_data(M, N, K, P)
    want_W, want_b = lb.wgrad_exact(g, x, P), lb.bias_grad_exact(g, P)
    gd, xd = _dev(g), _dev(x)
    rc, dW, db = _wgrad(gd, xd)
    assert rc == 0
    _same(dW, want_W, f"dW {M}x{N}x{K}")
    _same(db, want_b, f"db {M}x{N}x{K}")
    rc, dW2, db2 = _wgrad(gd, xd, ws_fill=0x00)
    assert rc == 0
    _same(dW2, dW, "dW, second run")
    _same(db2, db, "db, second run")
    assert not torch.isnan(dW).any() and torch.equal(gd.cpu(), torch.tensor(g)) and torch.equal(xd.cpu(), torch.tensor(x))


@pytest.mark.parametrize("rows", ["3", "P+1", "2P+3"])
@pytest.mark.parametrize("N,K", [(64, 64), (130, 36)])
def test_wgrad_four_bytes_off_alignment_gives_the_same_bits(N, K, rows):
    """N % 4 == 0 and K % 4 == 0: the aligned call takes the 16-byte sweeps, the offset one the 4-byte sweeps"""
    M = _rows(rows)
    P = lb.partition(M)
    g, x = lb.wgrad_data(M, N, K, P)
    rc, dW, db = _wgrad(_dev(g), _dev(x))
    rc1, dW1, db1 = _wgrad(_dev(g, 1), _dev(x, 1), offset=1)
    assert rc == 0 and rc1 == 0
    _same(dW1, dW, "dW off alignment")
    _same(db1, db, "db off alignment")
    _same(dW1, lb.wgrad_exact(g, x, P), "dW off alignment against the restatement")
    # one operand off: still the 4-byte sweeps
    rc2, dW2, _ = _wgrad(_dev(g), _dev(x, 1))
    assert rc2 == 0
    _same(dW2, dW, "dW, x alone off alignment")


@pytest.mark.parametrize("rows", ["3", "P+1"])
def test_wgrad_without_bias_gradient(rows):
    M, N, K = _rows(rows), 33, 31
    P = lb.partition(M)
    g, x = lb.wgrad_data(M, N, K, P)
    rc, dW, db = _wgrad(_dev(g), _dev(x), bias=False)
    assert rc == 0 and db is None
    _same(dW, lb.wgrad_exact(g, x, P), "dW with db NULL")


def test_wgrad_of_no_rows_is_zero():
    from pinsage_hip import native as nv
    N, K = 33, 31
    dW, db = _nan((N, K)), _nan((N,))
    assert nv.lib().ps_linear_wgrad(None, 0, N, None, K, nv.ptr(dW), nv.ptr(db), None, 0, nv.stream()) == 0
    assert not _host(dW).view(np.uint32).any() and not _host(db).view(np.uint32).any()


def test_wgrad_where_the_partition_doubles():
    """M = 256 * 512 + 1: the first row count with partitions of 1024 rows (129 of them); N = K = 33"""
    M, N, K = lb.doubling_rows(), 33, 33
    P = lb.partition(M)
    assert P == 2 * lb.partition(M - 1) == 2 * lb.PART
    g, x = lb.wgrad_data(M, N, K, P)
    rc, dW, db = _wgrad(_dev(g), _dev(x))
    assert rc == 0
    _same(dW, lb.wgrad_exact(g, x, P), "dW at the doubled partition")
    _same(db, lb.bias_grad_exact(g, P), "db at the doubled partition")
    # and not the bits of the undoubled rule (two columns of each operand suffice to tell)
    assert lb.mismatches(_host(dW)[:2, :2], lb.wgrad_exact(g[:, :2], x[:, :2], P // 2)) != []


def test_wgrad_error_codes():
    from pinsage_hip import native as nv
    P = lb.partition(1)
    M, N, K = P + 1, 8, 4
    g, x, dW, db = _dev(np.ones((M, N), np.float32)), _dev(np.ones((M, K), np.float32)), _nan((N, K)), _nan((N,))
    n = nv.lib().ps_linear_wgrad_workspace_bytes(M, N, K)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    f, st = nv.lib().ps_linear_wgrad, nv.stream()
    ok = [nv.ptr(g), M, N, nv.ptr(x), K, nv.ptr(dW), nv.ptr(db), nv.ptr(ws), n, st]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    assert call() == 0
    assert call(a2=0) == PS_EINVAL and call(a4=0) == PS_EINVAL and call(a1=-1) == PS_EINVAL
    assert call(a0=None) == PS_EINVAL and call(a3=None) == PS_EINVAL and call(a5=None) == PS_EINVAL
    assert call(a7=None) == PS_EINVAL and call(a8=n - 1) == PS_EWORKSPACE
    assert call(a1=P, a7=None, a8=0) == 0                                     # M <= P needs no workspace
    torch.cuda.synchronize()


# ---- 2: ps_linear_epilogue_bwd -------------------------------------------------------------------------------------------------------
def _epilogue(t, g, relu, l2, offset=0, in_place=False):
    from pinsage_hip import native as nv
    td, gd = _dev(t, offset), _dev(g, offset)
    gz = gd if in_place else _nan(t.shape, offset)
    flags = (nv.PS_RELU if relu else 0) | (nv.PS_L2NORM if l2 else 0)
    rc = nv.lib().ps_linear_epilogue_bwd(nv.ptr(td), nv.ptr(gd), t.shape[0], t.shape[1], flags, nv.ptr(gz), nv.stream())
    assert rc == 0
    assert torch.equal(td.cpu().view(torch.int32), torch.tensor(t).view(torch.int32))
    return gz


@pytest.mark.parametrize("relu,l2", lb.FLAGSETS)
@pytest.mark.parametrize("N", lb.EPILOGUE_N)
def test_epilogue_bwd_equals_the_restatement(N, relu, l2):
    """every row of epilogue_data: plain rows, the all-zero row, the rows just above and just below the clamp, the NaN row"""
    t, g, rows = lb.epilogue_data(N)
    want = lb.epilogue_bwd_exact(t, g, relu, l2, lb.vec_of(N))
    _same(_epilogue(t, g, relu, l2), want, f"gz N={N}")
    _same(_epilogue(t, g, relu, l2, in_place=True), want, f"gz in place N={N}")
    _same(_epilogue(t, g, relu, l2, offset=1), lb.epilogue_bwd_exact(t, g, relu, l2, 1), f"gz 4 bytes off N={N}")
    _same(_epilogue(t, g, relu, l2, offset=1, in_place=True), lb.epilogue_bwd_exact(t, g, relu, l2, 1), f"gz 4 bytes off, in place N={N}")


@pytest.mark.parametrize("N", [4, 65, 300])
def test_epilogue_bwd_planted_rows(N):
    t, g, rows = lb.epilogue_data(N)
    z, a, b, n = (rows[k] for k in ("zero_row", "above_row", "below_row", "nan_row"))
    full, nomask = _host(_epilogue(t, g, True, True)), _host(_epilogue(t, g, False, True))
    assert not full[z].view(np.uint32).any()                                  # g / 1e-12 masked by the ReLU: +0 bits
    _same(nomask[z], (g[z] / lb.CLAMP).astype(np.float32), "zero row without the mask")
    _same(nomask[b], (g[b] / lb.CLAMP).astype(np.float32), "row below the clamp")
    assert nomask[a, N - 1] == 0
    _same(nomask[a, :N - 1], (g[a, :N - 1] / np.float32(2.0 ** -39)).astype(np.float32), "row above the clamp")
    # a NaN in t makes its row NaN (under the ReLU: wherever t > 0, as the header defines the mask) and no other
    assert np.isnan(nomask[n]).all() and (np.isnan(full[n]) == (t[n] > 0)).all()
    rest = [r for r in range(t.shape[0]) if r != n]
    assert not np.isnan(nomask[rest]).any() and not np.isnan(full[rest]).any()
    clean = np.array(t)
    clean[n, N - 1] = 1.0
    _same(_host(_epilogue(clean, g, False, True))[rest], nomask[rest], "the rows beside the NaN row")


def test_epilogue_bwd_error_codes_and_empty():
    from pinsage_hip import native as nv
    t, g, _ = lb.epilogue_data(4)
    td, gd, gz = _dev(t), _dev(g), _nan(t.shape)
    f, st = nv.lib().ps_linear_epilogue_bwd, nv.stream()
    M, N = t.shape
    assert f(nv.ptr(td), nv.ptr(gd), M, N, 4, nv.ptr(gz), st) == PS_EINVAL
    assert f(nv.ptr(td), nv.ptr(gd), M, 0, 3, nv.ptr(gz), st) == PS_EINVAL
    assert f(nv.ptr(td), nv.ptr(gd), -1, N, 3, nv.ptr(gz), st) == PS_EINVAL
    assert f(None, nv.ptr(gd), M, N, 3, nv.ptr(gz), st) == PS_EINVAL
    assert f(nv.ptr(td), None, M, N, 3, nv.ptr(gz), st) == PS_EINVAL
    assert f(nv.ptr(td), nv.ptr(gd), M, N, 3, None, st) == PS_EINVAL
    assert f(None, None, 0, N, 3, None, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(gz).all()


# ---- 3: dense.linear on the tape -----------------------------------------------------------------------------------------------------
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
        out, self.names = self.names, []
        return out


LEAVES = ("x", "W", "b", "x2", "W2")
LAYER = (None, 16, 12, 8)                    # M = P + 40 (two partitions: the workspace), K, N, K2


def _layer():
    M = lb.partition(1) + 40
    return M, lb.layer_data(M, *LAYER[1:])


def _linear_step(d, need, relu, l2, G):
    from pinsage_hip import dense
    ls = {k: torch.tensor(d[k]).cuda().requires_grad_(k in need) for k in LEAVES}
    y = dense.linear(ls["x"], ls["W"], ls["b"], x2=ls["x2"], W2=ls["W2"], relu=relu, l2norm=l2)
    if need:
        y.backward(G)
    return y, {k: ls[k].grad for k in LEAVES}


@pytest.mark.parametrize("relu,l2", lb.FLAGSETS)
def test_linear_is_differentiable(relu, l2, monkeypatch):
    """Every subset of {x, W, b, x2, W2} requiring a gradient.  On the parent commit dense.linear returns a tensor without a
    grad_fn here, and backward() raises."""
    from pinsage_hip import dense, sampling
    M, d = _layer()
    P = lb.partition(M)
    bounds, ref = lb.layer_grad_bounds(d["x"], d["W"], d["b"], d["x2"], d["W2"], d["G"], relu, l2, P)
    G = torch.tensor(d["G"]).cuda()
    with torch.no_grad():
        y_inf = dense.linear(*(torch.tensor(d[k]).cuda() for k in ("x", "W", "b")), x2=torch.tensor(d["x2"]).cuda(),
                             W2=torch.tensor(d["W2"]).cuda(), relu=relu, l2norm=l2)
        t_inf = dense.linear(*(torch.tensor(d[k]).cuda() for k in ("x", "W", "b")), x2=torch.tensor(d["x2"]).cuda(),
                             W2=torch.tensor(d["W2"]).cuda(), relu=relu)
    spy = _Spy(monkeypatch)
    for r in range(len(LEAVES) + 1):
        for need in itertools.combinations(LEAVES, r):
            spy.take()
            y, grads = _linear_step(d, need, relu, l2, G)
            called = spy.take()
            what = f"relu={relu} l2norm={l2} need={need}"
            if not need:
                assert y.grad_fn is None and not set(called) & NEW, what
                _same(y, y_inf, what + ": the inference call")
                continue
            assert y.grad_fn is not None and y.requires_grad, what
            # the forward: the inference call's bits before the norm, within gemm_cases.norm_bound of its float64 quotient after
            if l2:
                assert gc.mismatches_normed(_host(y), _host(t_inf), gc.ref_normed(_host(t_inf))) == [], what
            else:
                _same(y, y_inf, what + ": forward")
            for k in LEAVES:
                assert (grads[k] is not None) == (k in need), (what, k)
                if k in need:
                    assert lb.outside(_host(grads[k]), ref[k], bounds[k]) == [], (what, k)
            # which entry points made them: one weight-gradient GEMM per weight (the bias rides on W's, or takes one of its own)
            n_wgrad = ("W" in need) + ("W2" in need) + ("b" in need and "W" not in need)
            assert called.count("ps_linear_wgrad") == n_wgrad, (what, called)
            assert called.count("ps_linear_epilogue_bwd") == int(relu or l2), (what, called)
            assert called.count("ps_linear") == 1 + ("x" in need) + ("x2" in need), (what, called)
            y2, grads2 = _linear_step(d, need, relu, l2, G)
            _same(y2, y, what + ": two passes, y")
            for k in need:
                _same(grads2[k], grads[k], what + f": two passes, d{k}")
    # the torch method on the same leaves: no new entry point, the same gradients within the bound
    monkeypatch.setattr(sampling, "grad_method", "torch")
    spy.take()
    y_t, grads_t = _linear_step(d, LEAVES, relu, l2, G)
    assert not set(spy.take()) & (NEW | {"ps_linear"})
    monkeypatch.setattr(sampling, "grad_method", "hip")
    y_h, grads_h = _linear_step(d, LEAVES, relu, l2, G)
    for k in LEAVES:
        assert lb.outside(_host(grads_h[k]), _host(grads_t[k]).astype(np.float64), bounds[k]) == [], k
        assert lb.outside(_host(grads_t[k]), ref[k], bounds[k]) == [], k


def test_linear_single_operand_without_bias_and_staged_weights():
    from pinsage_hip import dense
    d = lb.layer_data(70, 32, 12, 0, bias=False)
    P = lb.partition(70)
    bounds, ref = lb.layer_grad_bounds(d["x"], d["W"], None, None, None, d["G"], True, True, P)
    x, W = (torch.tensor(d[k]).cuda().requires_grad_(True) for k in ("x", "W"))
    y = dense.linear(x, W, relu=True, l2norm=True)
    y.backward(torch.tensor(d["G"]).cuda())
    for k, t in (("x", x), ("W", W)):
        assert lb.outside(_host(t.grad), ref[k], bounds[k]) == [], k
    # a column slice of a leaf as the weight: the gradient reaches the leaf, zero outside the slice
    big = torch.zeros((12, 40), device="cuda")
    big[:, 4:36] = torch.tensor(d["W"]).cuda()
    big.requires_grad_(True)
    dense.linear(x.detach(), big[:, 4:36], relu=True, l2norm=True).backward(torch.tensor(d["G"]).cuda())
    _same(big.grad[:, 4:36], W.grad, "the gradient of a column slice")
    assert not big.grad[:, :4].any() and not big.grad[:, 36:].any()
    staged = dense.stage_weight(W.detach())
    assert isinstance(staged, dense.StagedWeight)
    with pytest.raises(ValueError):
        dense.linear(x, staged)
    with torch.no_grad():
        _same(dense.linear(x, staged), dense.linear(x, W), "staged weights off the tape")
    with pytest.raises(RuntimeError):                                         # once-differentiable
        xx = x.detach().requires_grad_(True)
        gx, = torch.autograd.grad(dense.linear(xx, W.detach(), relu=True, l2norm=True).sum(), xx, create_graph=True)
        gx.sum().backward()


# ---- 4: the three PinSage branches -----------------------------------------------------------------------------------------------------
def _model_case(branch):
    rs = np.random.RandomState({"mlp": 51, "edge": 52, "pooled": 53}[branch])
    n = 300
    x = torch.tensor(rs.random_sample((n, 16)).astype(np.float32) + 0.5, device="cuda")
    if branch == "mlp":
        return x, {}
    if branch == "edge":
        ei = torch.tensor(np.stack([rs.randint(0, n, 2000), rs.randint(0, n, 2000)]), dtype=torch.int64, device="cuda")
        return x, {"edge_index": ei}
    nb = [[int(j) for j in rs.randint(0, n, rs.randint(0, 6))] for _ in range(n)]
    wt = [[float(w) for w in rs.random_sample(len(r)) + 0.1] for r in nb]
    return x, {"sampled_neighbors": [nb, nb], "importance_weights": [wt, wt]}


def _model_step(model, x, kw, spy):
    model.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(True)
    spy.take()
    out = model(xx, **kw)
    fwd = set(spy.take())
    out.backward(torch.tensor(np.random.RandomState(41).standard_normal(tuple(out.shape)).astype(np.float32), device="cuda"))
    bwd = set(spy.take())
    return [out.detach(), xx.grad] + [None if p.grad is None else p.grad.clone() for p in model.parameters()], fwd, bwd


@pytest.mark.parametrize("branch", ["mlp", "edge", "pooled"])
def test_pinsage_branch_takes_a_training_step(branch, monkeypatch):
    """16 -> 32 -> 8, two layers, 300 rows.  A branch that model.pinsage.HIP_LINEAR leaves on torch (its step measured slower than
    the torch method's: DESIGN.md §4, "Dense layers, training") must call none of the new entry points; the others must."""
    import model.pinsage as pin
    from pinsage_hip import sampling
    torch.manual_seed(7)
    model = pin.PinSage(16, 32, 8, 2).cuda()
    x, kw = _model_case(branch)
    spy = _Spy(monkeypatch)
    a, fwd, bwd = _model_step(model, x, kw, spy)
    b, _, _ = _model_step(model, x, kw, spy)
    if pin.HIP_LINEAR[branch]:
        assert "ps_linear" in fwd and "ps_bn_apply" in fwd and NEW <= bwd and "ps_linear" in bwd, (fwd, bwd)
    else:
        assert not (fwd | bwd) & (NEW | {"ps_linear"}), (fwd, bwd)
    used = {n for n, p in model.named_parameters() if p.grad is not None}
    assert a[1] is not None and {"input_proj.weight", "convs.1.lin_self.bias", "output_proj.weight"} <= used
    assert ("convs.0.lin_update.weight" in used) == (branch != "mlp") and ("convs.0.lin_neigh.weight" in used) == (branch == "edge")
    for p, q in zip(a, b):
        assert (p is None) == (q is None)
        if p is not None:
            _same(p, q, f"{branch}: two passes")
    monkeypatch.setattr(sampling, "grad_method", "torch")
    r, rf, rb = _model_step(model, x, kw, spy)
    monkeypatch.setattr(sampling, "grad_method", "hip")
    assert not (rf | rb) & (NEW | {"ps_linear"})
    for p, q in zip(a, r):
        assert (p is None) == (q is None)
        if p is None:
            continue
        np.testing.assert_allclose(_host(p), _host(q), rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=f"{branch} against the torch method")
    # inference: no new entry point, and the bits of the code as it was (every switch of the new routing off)
    spy.take()
    with torch.no_grad():
        o = model(x, **kw)
    assert not set(spy.take()) & NEW
    monkeypatch.setattr(pin, "HIP_LINEAR", dict.fromkeys(pin.HIP_LINEAR, False))
    with torch.no_grad():
        o_before = model(x, **kw)
    _same(o, o_before, f"{branch}: no_grad forward")
    np.testing.assert_allclose(_host(o), _host(a[0]), rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=f"{branch}: inference against training forward")
