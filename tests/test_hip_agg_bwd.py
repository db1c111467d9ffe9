"""The backward kernels of the neighbour gathers (csrc/neigh_agg_bwd.hip) on the GPU:

  1. every entry point equals the numpy restatement of tests/helpers/agg_bwd_cases.py bit for bit, and itself on a second run;
  2. ps_importance_pool(x, wts = w_eff, renorm = 0) repeats the forward's bits;
  3. the autograd Functions of pinsage_hip.sampling against torch autograd of the same expression on the same leaf tensors;
  4. the modules against sampling.grad_method = "torch";
  5. AttentionAggregator's forward + backward stays below one [B, T, C] tensor of peak allocation;
  6. argument errors and empty problems.

Outputs are filled with NaN before every raw call."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import agg_bwd_cases as bc  # noqa: E402
import agg_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-5           # tests/test_hip_model.py's gradient tolerance
NONEMPTY = [ci for ci in range(bc.N_CASES) if ci >= len(bc.CASES) or bc.CASES[ci][0] > 0]      # B = 0: test_empty_problems
CASE_IDS = [f"c{ci}-B{c[0]}-H{c[2]}-T{c[3]}" + ("-offset" if c[4] else "") for ci, c in enumerate(bc.CASES)] + ["hub-a", "hub-b"]


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
    assert t.is_contiguous() and (a.size == 0 or t.data_ptr() % 16 != 0)
    return t


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(np.argwhere(bad)[0])}"


def _ws(fn, *dims):
    from pinsage_hip import native as nv
    n = getattr(nv.lib(), fn)(*dims)
    return torch.empty(max(n, 1), dtype=torch.uint8, device="cuda"), n


def _raw_pool_weights(ids, counts, wts, nvalid, max_idx, renorm, lanes):
    from pinsage_hip import native as nv
    B, T = ids.shape
    w = _nan(B, T)
    nv.call("ps_pool_weights", nv.ptr(ids), nv.ptr(counts), nv.ptr(wts), nv.ptr(nvalid), B, T, max_idx, int(renorm), lanes,
            nv.ptr(w), nv.stream())
    return w


def _raw_gather_bwd(rptr, slots, N, T, g, coef=None, arg=None):
    from pinsage_hip import native as nv
    B, H = g.shape
    gx = _nan(N, H)
    ws, n = _ws("ps_gather_bwd_workspace_bytes", B, T, H)
    ws.fill_(0xff)
    nv.call("ps_gather_bwd", nv.ptr(rptr), nv.ptr(slots), N, T, nv.ptr(coef), nv.ptr(arg), nv.ptr(g), B, H, nv.ptr(gx),
            nv.ptr(ws), n, nv.stream())
    return gx


def _raw_max_arg(x, ids, nvalid):
    from pinsage_hip import native as nv
    B, T = ids.shape
    N, H = x.shape
    out = _nan(B, H)
    arg = torch.full((B, H), -7, dtype=torch.int32, device="cuda")
    nv.call("ps_gather_max_arg", nv.ptr(x), N, H, nv.ptr(ids), nv.ptr(nvalid), B, T, nv.ptr(out), nv.ptr(arg), nv.stream())
    return out, arg


def _raw_attention_rows(x, u, v, w2, ids, nvalid, attn, g):
    from pinsage_hip import native as nv
    B, T = ids.shape
    N, H = x.shape
    Hd = v.shape[1]
    ds, du, dw2 = _nan(B, T), _nan(B, Hd), _nan(Hd)
    ws, n = _ws("ps_attention_bwd_rows_workspace_bytes", B, Hd)
    ws.fill_(0xff)
    nv.call("ps_attention_bwd_rows", nv.ptr(x), N, H, nv.ptr(u), nv.ptr(v), Hd, nv.ptr(w2), nv.ptr(ids), nv.ptr(nvalid),
            nv.ptr(attn), nv.ptr(g), B, T, nv.ptr(ds), nv.ptr(du), nv.ptr(dw2), nv.ptr(ws), n, nv.stream())
    return ds, du, dw2


def _raw_attention_cols(rptr, slots, N, T, ds, u, v, w2):
    from pinsage_hip import native as nv
    B, Hd = u.shape
    dv = _nan(N, Hd)
    ws, n = _ws("ps_gather_bwd_workspace_bytes", B, T, Hd)
    ws.fill_(0xff)
    nv.call("ps_attention_bwd_cols", nv.ptr(rptr), nv.ptr(slots), N, T, nv.ptr(ds), nv.ptr(u), nv.ptr(v), Hd, nv.ptr(w2), B,
            nv.ptr(dv), nv.ptr(ws), n, nv.stream())
    return dv


# ---- 1: bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(bc.N_CASES), ids=CASE_IDS)
def test_pool_backward_bit_exact(ci):
    from pinsage_hip import sampling
    c = bc.case(ci)
    o, N, T, top = c["offset"], c["N"], c["T"], c["max_idx"]
    ids, nvalid, g = _dev(c["ids"]), _dev(c["nvalid"]), _dev(c["g"], o)
    keep = bc.kept_pool(c["ids"], c["nvalid"], top)
    rptr_ref, slots_ref = bc.slot_lists_ref(c["ids"], keep, N)
    rptr, slots = sampling.slot_lists(ids, nvalid, N, top)
    assert np.array_equal(rptr.cpu().numpy(), rptr_ref) and np.array_equal(slots.cpu().numpy()[:len(slots_ref)], slots_ref)
    assert rptr.dtype == torch.int64 and slots.dtype == torch.int32
    for lanes in (16, 64):
        for use_counts, renorm in ((True, True), (True, False), (False, True), (False, False)):
            cn = _dev(c["counts"]) if use_counts else None
            wt = None if use_counts else _dev(c["wts"], o)
            want = bc.pool_weights_exact(c["ids"], c["counts"] if use_counts else None, None if use_counts else c["wts"],
                                         c["nvalid"], top, renorm, lanes)
            w = _raw_pool_weights(ids, cn, wt, nvalid, top, renorm, lanes)
            _same(w, want, f"case {ci} w_eff lanes {lanes} counts {use_counts} renorm {renorm}")
            _same(_raw_pool_weights(ids, cn, wt, nvalid, top, renorm, lanes), w, "w_eff, second run")
    if c["B"] == 0:
        gx = _raw_gather_bwd(rptr, slots, N, T, g, coef=w)
        assert not _bits(gx).any()
        return
    gx = _raw_gather_bwd(rptr, slots, N, T, g, coef=w)
    _same(gx, bc.gather_bwd_exact(rptr_ref, slots_ref, N, T, c["g"], coef=want), f"case {ci} gx")
    _same(_raw_gather_bwd(rptr, slots, N, T, g, coef=w), gx, "gx, second run")
    assert not _bits(gx)[np.diff(rptr_ref) == 0].any()        # +0.0 where nothing points


@pytest.mark.parametrize("ci", NONEMPTY, ids=[CASE_IDS[ci] for ci in NONEMPTY])
def test_max_backward_bit_exact(ci):
    from pinsage_hip import sampling
    c = bc.case(ci)
    o, N, T = c["offset"], c["N"], c["T"]
    for plant_nan in (False, True):
        xh = c["x"].copy()
        if plant_nan:                                             # two NaNs in one column of a list, and a -inf
            xh[int(c["ids"][min(2, c["B"] - 1), 0]), 1] = np.nan
            xh[int(c["ids"][0, 0]), 0] = -np.inf
            if T >= 3 and c["B"] == 50:
                xh[17, 2] = np.nan
        x, ids, nvalid, g = _dev(xh, o), _dev(c["ids"]), _dev(c["nvalid"]), _dev(c["g"], o)
        want_out, want_arg = bc.gather_max_arg_ref(xh, c["ids"], c["nvalid"])
        out, arg = _raw_max_arg(x, ids, nvalid)
        got_arg = arg.cpu().numpy()
        bad = np.argwhere(got_arg != want_arg)
        assert not len(bad), f"case {ci} arg (NaN planted: {plant_nan}): {len(bad)} differ, first (row, column) {tuple(bad[0])}: " \
                             f"{got_arg[tuple(bad[0])]} for {want_arg[tuple(bad[0])]}, list {c['ids'][bad[0][0]]}"
        _same(out, sampling.gather_max(x, ids, nvalid), f"case {ci}: out against ps_gather_max")
        if not plant_nan:
            _same(out, want_out, f"case {ci} max out")
        else:
            assert np.array_equal(np.isnan(out.cpu().numpy()), np.isnan(want_out))
        keep = ac.kept(c["ids"], c["nvalid"], N)
        rptr_ref, slots_ref = bc.slot_lists_ref(c["ids"], keep, N)
        rptr, slots = sampling.slot_lists(ids, nvalid, N)
        assert np.array_equal(rptr.cpu().numpy(), rptr_ref) and np.array_equal(slots.cpu().numpy()[:len(slots_ref)], slots_ref)
        gx = _raw_gather_bwd(rptr, slots, N, T, g, arg=arg)
        _same(gx, bc.gather_bwd_exact(rptr_ref, slots_ref, N, T, c["g"], arg=want_arg), f"case {ci} max gx")
        _same(_raw_gather_bwd(rptr, slots, N, T, g, arg=arg), gx, "max gx, second run")


@pytest.mark.parametrize("ci", NONEMPTY, ids=[CASE_IDS[ci] for ci in NONEMPTY])
def test_attention_backward_bit_exact(ci):
    from pinsage_hip import sampling
    c = bc.case(ci)
    o, N, T, vec = c["offset"], c["N"], c["T"], c["vec"]
    x, u, v, w2, g = (_dev(c[k], o) for k in ("x", "u", "v", "w2", "g"))
    ids, nvalid = _dev(c["ids"]), _dev(c["nvalid"])
    attn = sampling.attention_weights(u, v, w2, ids, nvalid)
    attn_h = attn.cpu().numpy()
    keep = ac.kept(c["ids"], c["nvalid"], N)
    want_ds, want_du, want_dw2, _ = bc.attention_bwd_rows_exact(c["x"], c["u"], c["v"], c["w2"], c["ids"], c["nvalid"], attn_h,
                                                                c["g"], vec)
    ds, du, dw2 = _raw_attention_rows(x, u, v, w2, ids, nvalid, attn, g)
    _same(ds, want_ds, f"case {ci} ds")
    _same(du, want_du, f"case {ci} du")
    _same(dw2, want_dw2, f"case {ci} dw2")
    assert not _bits(ds)[~keep].any()
    again = _raw_attention_rows(x, u, v, w2, ids, nvalid, attn, g)
    for a, b, name in zip(again, (ds, du, dw2), ("ds", "du", "dw2")):
        _same(a, b, f"{name}, second run")
    rptr_ref, slots_ref = bc.slot_lists_ref(c["ids"], keep, N)
    rptr, slots = sampling.slot_lists(ids, nvalid, N)
    dv = _raw_attention_cols(rptr, slots, N, T, ds, u, v, w2)
    _same(dv, bc.attention_bwd_cols_exact(rptr_ref, slots_ref, N, T, want_ds, c["u"], c["v"], c["w2"]), f"case {ci} dv")
    _same(_raw_attention_cols(rptr, slots, N, T, ds, u, v, w2), dv, "dv, second run")
    dx = _raw_gather_bwd(rptr, slots, N, T, g, coef=attn)
    _same(dx, bc.gather_bwd_exact(rptr_ref, slots_ref, N, T, c["g"], coef=attn_h), f"case {ci} dx")


# ---- 2: w_eff repeats the forward ----------------------------------------------------------------------------------------------
def _forward_lanes(x, out):
    return 16 if x.size(1) % 4 == 0 and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 else 64


def test_pool_weights_repeat_the_forward(golden):
    from pinsage_hip import sampling
    rs = np.random.RandomState(11)
    shapes = []
    g = golden
    for tag in ("items", "all"):                                # the pooling goldens' shapes: given weights, ids beyond the rows
        h = g[f"g2_h_{tag}"]
        shapes.append((h, g["g2_ids"].astype(np.int32), None, g["g2_weights"].astype(np.float32), g["g2_nvalid"], h.shape[0] - 1))
    # tests/test_hip_model.py's fuzz table, the rows with T > 16 and its neighbours, plus a scalar-sweep width
    for T, H, B, N in [(17, 100, 66, 300), (50, 256, 513, 2000), (64, 512, 65, 70), (65, 64, 40, 60), (16, 260, 130, 90), (17, 33, 40, 60)]:
        x = rs.standard_normal((N, H)).astype(np.float32)
        ids = rs.randint(-1, N + N // 3 + 1, size=(B, T)).astype(np.int32)
        nvalid = rs.randint(0, T + 1, size=B).astype(np.int32)
        nvalid[rs.randint(0, B, size=max(1, B // 10))] = 0
        counts = rs.randint(1, 30, size=(B, T)).astype(np.int32)
        wts = (rs.random_sample((B, T)) + 0.05).astype(np.float32)
        shapes.append((x, ids, counts, wts, nvalid, N - 1 - rs.randint(0, 5)))
    seen = set()
    for x, ids, counts, wts, nvalid, max_idx in shapes:
        xt, it, nt = _dev(x), _dev(ids), _dev(nvalid)
        for use_counts in ((True, False) if counts is not None else (False,)):
            for renorm in (True, False):
                cn = _dev(counts) if use_counts else None
                wt = None if use_counts else _dev(wts)
                fwd = sampling.importance_pool(xt, ids=it, counts=cn, wts=wt, nvalid=nt, max_idx=max_idx, renorm=renorm)
                lanes = _forward_lanes(xt, fwd)
                seen.add((lanes, ids.shape[1] > 16))
                w = sampling.pool_weights(it, cn, wt, nt, max_idx, renorm, lanes)
                again = sampling.importance_pool(xt, ids=it, wts=w, nvalid=nt, max_idx=max_idx, renorm=False)
                _same(again, fwd, f"T {ids.shape[1]} H {x.shape[1]} counts {use_counts} renorm {renorm} lanes {lanes}")
    assert (16, True) in seen and (64, True) in seen


# ---- 3: the Functions against torch autograd on the same leaves ------------------------------------------------------------------
def _grads(fn, leaves, need, g=None):
    """gradients of fn(*leaves) with respect to the leaves flagged in `need` (None for the others)"""
    ls = [t.detach().clone().requires_grad_(n) for t, n in zip(leaves, need)]
    out = fn(*ls)
    if g is None:
        out.sum().backward()                                      # hands the backward a stride-0 gradient
    else:
        out.backward(g)
    return out.detach(), [t.grad for t in ls]


def _close(a, b, what):
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=what)


def _function_case(ci):
    c = bc.case(ci)
    xh = c["x"].copy()
    xh[85] = xh[84] + np.float32(0.25)                           # torch.max breaks ties between distinct ids its own way
    return c, xh


@pytest.mark.parametrize("ci", (0, 1, 3))
def test_functions_against_torch_autograd(ci):
    from pinsage_hip import sampling
    assert sampling.grad_method == "hip"
    c, xh = _function_case(ci)
    x, u, v, w2, g = _dev(xh), _dev(c["u"]), _dev(c["v"]), _dev(c["w2"]), _dev(c["g"])
    b2 = torch.tensor([0.3], device="cuda")
    ids, nvalid = _dev(c["ids"]), _dev(c["nvalid"])
    # pool: the torch expression multiplies by the weights the kernel used, so the masks are identical by construction
    for use_counts, renorm in ((True, True), (False, False)):
        cn = _dev(c["counts"]) if use_counts else None
        wt = None if use_counts else _dev(c["wts"])
        fwd = sampling.importance_pool(x, ids=ids, counts=cn, wts=wt, nvalid=nvalid, max_idx=c["max_idx"], renorm=renorm)
        w = sampling.pool_weights(ids, cn, wt, nvalid, c["max_idx"], renorm, _forward_lanes(x, fwd))
        idt = torch.where(w != 0, ids, torch.zeros_like(ids)).long()

        def pool_torch(xx):
            return (xx[idt] * w[:, :, None]).sum(dim=1)

        def pool_hip(xx):
            return sampling.pool(xx, ids=ids, counts=cn, wts=wt, nvalid=nvalid, max_idx=c["max_idx"], renorm=renorm)
        for gg in (g, None):
            o1, (g1,) = _grads(pool_hip, [x], [True], gg)
            o2, (g2,) = _grads(pool_torch, [x], [True], gg)
            _close(o1, o2, "pool out")
            _close(g1, g2, "pool dx")
    for gg in (g, None):
        o1, (g1,) = _grads(lambda xx: sampling.max_pool(xx, ids, nvalid), [x], [True], gg)
        o2, (g2,) = _grads(lambda xx: sampling.max_pool_torch(xx, ids, nvalid), [x], [True], gg)
        assert np.array_equal(o1.cpu().numpy(), o2.cpu().numpy())
        _close(g1, g2, "max dx")
    leaves = [x, u, v, w2, b2]
    names = ("x", "u", "v", "w2", "b2")
    for need in itertools.product((False, True), repeat=5):
        if not any(need):
            continue
        gg = g if sum(need) % 2 else None
        o1, g1 = _grads(lambda *ls: sampling.attention(*ls, ids, nvalid), leaves, need, gg)
        o2, g2 = _grads(lambda *ls: sampling.attention_torch(*ls, ids, nvalid), leaves, need, gg)
        _close(o1, o2, "attention out")
        for name, n, a, b in zip(names, need, g1, g2):
            if not n:
                assert a is None, f"{name} is frozen and received a gradient"
            elif name == "b2":
                assert a is not None and a.shape == b2.shape and not a.any()
            else:
                _close(a, b, f"attention d{name} with {need}")


# ---- 4: the modules against grad_method = "torch" --------------------------------------------------------------------------------
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


def _module_run(module, args, feats):
    """(out, feature grads, parameter grads) of one forward + backward"""
    module.zero_grad(set_to_none=True)
    fs = [f.detach().clone().requires_grad_(True) for f in feats]
    out = module(*args(fs))
    out.square().sum().backward()
    return out.detach(), [f.grad for f in fs], [p.grad.clone() for p in module.parameters()]


@pytest.mark.parametrize("ci", (2, 3))
def test_modules_against_torch_method(ci, monkeypatch):
    """agg_cases.case(2) and case(3): the smallest module shapes that take the 16-byte sweep (C = 8) and the scalar sweep
    (C = 10).  Larger shapes add no branch here -- the kernels' branches are the bit-exact tests' -- and the comparison itself
    degrades with size: the second attention layer's bias has an exactly zero gradient, which the HIP path returns and the
    torch method only approximates by a sum of B * T cancelling terms (at case(5), C = 260 and T = 64, torch's value is
    -1.1e-5, its own rounding noise, just beyond the absolute tolerance)."""
    from model import layers as L
    from pinsage_hip import sampling
    c = ac.case(ci)
    at, mp = ac.modules(ci)
    at.cuda(), mp.cuda()
    x, sx = _dev(c["x"]), _dev(c["self_x"])
    nb = c["neighbors"]
    spy = _Spy(monkeypatch)
    runs = (("attention", at, lambda fs: (fs[0], nb, fs[1]), [x, sx]),
            ("max aggregator", mp, lambda fs: (fs[0], nb), [x]),
            ("max layer", L.MaxPoolingLayer(), lambda fs: (fs[0], nb), [x]))
    called = set()
    for name, module, args, feats in runs:
        assert sampling.grad_method == "hip"
        spy.take()
        hip = _module_run(module, args, feats)
        called |= set(spy.take())
        hip2 = _module_run(module, args, feats)
        for a, b in zip([hip[0]] + hip[1] + hip[2], [hip2[0]] + hip2[1] + hip2[2]):
            _same(a, b, f"{name}: two passes")
        monkeypatch.setattr(sampling, "grad_method", "torch")
        spy.take()
        ref = _module_run(module, args, feats)
        torch_calls = set(spy.take())
        monkeypatch.setattr(sampling, "grad_method", "hip")
        assert not torch_calls & {"ps_gather_max_arg", "ps_gather_bwd", "ps_attention_bwd_rows", "ps_attention_bwd_cols"}, name
        _close(hip[0], ref[0], f"{name} out")
        if name == "attention":                                   # parameters(): ..., attention.2.weight, attention.2.bias
            assert hip[2][-1].shape == (1,) and not hip[2][-1].any()
        for a, b in zip(hip[1] + hip[2], ref[1] + ref[2]):
            _close(a, b, f"{name} gradients")
    assert {"ps_gather_max_arg", "ps_gather_bwd", "ps_attention_bwd_rows", "ps_attention_bwd_cols"} <= called


def test_pool_function_serves_the_weighted_modules(monkeypatch):
    """PoolFn.backward behind ImportancePooling: ps_pool_weights + ps_gather_bwd, the same gradient as the torch code, the same
    bits twice"""
    from model.pinsage import ImportancePooling
    from pinsage_hip import sampling
    torch.manual_seed(0)
    x = torch.randn(40, 24, device="cuda")
    nb = [[int(v) for v in np.random.RandomState(i).randint(0, 60, size=i % 7)] for i in range(40)]
    wt = [[float(v) for v in np.random.RandomState(100 + i).random_sample(i % 7) + 0.1] for i in range(40)]
    spy = _Spy(monkeypatch)

    def run():
        xx = x.clone().requires_grad_(True)
        ImportancePooling()(xx, nb, wt).pow(2).sum().backward()
        return xx.grad
    a, names = run(), spy.take()
    assert "ps_pool_weights" in names and "ps_gather_bwd" in names
    _same(run(), a, "two passes")
    monkeypatch.setattr(sampling, "grad_method", "torch")
    spy.take()
    b = run()
    assert "ps_gather_bwd" not in spy.take()
    _close(a, b, "ImportancePooling dx")


# ---- 5: peak allocation ----------------------------------------------------------------------------------------------------------
def test_attention_training_builds_no_padded_float_tensor(monkeypatch):
    """B = N = 4096, C = 64, T = 32, forward + backward: below ONE [B, T, C] fp32 tensor with the HIP backward (its own tensors --
    u, v, their gradients, dx, attn, ds, the slot lists and the sort behind them -- are about 12 MB against 33 MB); the torch
    method builds at least two"""
    from model import aggregators as A
    from pinsage_hip import sampling
    B = N = 4096
    C, T = 64, 32
    rs = np.random.RandomState(11)
    x = _dev(rs.standard_normal((N, C)).astype(np.float32))
    nb = rs.randint(0, N, size=(B, T)).tolist()
    torch.manual_seed(5)
    at = A.AttentionAggregator(C).cuda()

    def peak():
        at.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = at(xx, nb)
        out.square().sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, xx.grad
    peak()                                                        # warm-up: library handles, the allocator's first blocks
    grew, gx = peak()
    monkeypatch.setattr(sampling, "grad_method", "torch")
    grew_torch, gx_torch = peak()
    print(f"peak allocation: HIP backward {grew} bytes, torch method {grew_torch} bytes; one [B,T,C] tensor {4 * B * T * C}")
    assert grew < 4 * B * T * C
    assert grew_torch >= 8 * B * T * C
    _close(gx, gx_torch, "dx at the large shape")


# ---- 6: errors and empty problems ------------------------------------------------------------------------------------------------
def test_argument_errors():
    from pinsage_hip import native as nv
    lib = nv.lib()
    c = bc.case(0)
    B, N, H, T = c["B"], c["N"], c["H"], c["T"]
    ids, nvalid, cn = _dev(c["ids"]), _dev(c["nvalid"]), _dev(c["counts"])
    x, u, v, w2, g = (_dev(c[k]) for k in ("x", "u", "v", "w2", "g"))
    w, gx, arg = _nan(B, T), _nan(N, H), torch.zeros((B, H), dtype=torch.int32, device="cuda")
    rptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    slots = torch.zeros(B * T, dtype=torch.int32, device="cuda")
    ws, n = _ws("ps_gather_bwd_workspace_bytes", B, T, H)
    wr, nr = _ws("ps_attention_bwd_rows_workspace_bytes", B, H)
    p, st, null = nv.ptr, nv.stream(), nv.ptr(None)
    E = nv.PS_EINVAL
    assert lib.ps_gather_bwd_segment() == bc.segment() > 0
    assert lib.ps_pool_weights(p(ids), p(cn), null, p(nvalid), B, 0, N - 1, 1, 16, p(w), st) == E
    assert lib.ps_pool_weights(p(ids), p(cn), null, p(nvalid), B, T, N - 1, 1, 32, p(w), st) == E
    assert lib.ps_pool_weights(p(ids), null, null, p(nvalid), B, T, N - 1, 1, 16, p(w), st) == E
    assert lib.ps_pool_weights(p(ids), p(cn), null, p(nvalid), B, T, N - 1, 1, 16, null, st) == E
    assert lib.ps_gather_bwd(p(rptr), p(slots), N, T, p(w), null, p(g), B, 0, p(gx), p(ws), n, st) == E
    assert lib.ps_gather_bwd(p(rptr), p(slots), N, T, p(w), p(arg), p(g), B, H, p(gx), p(ws), n, st) == E      # both given
    assert lib.ps_gather_bwd(p(rptr), p(slots), N, T, null, null, p(g), B, H, p(gx), p(ws), n, st) == E        # neither
    assert lib.ps_gather_bwd(null, p(slots), N, T, p(w), null, p(g), B, H, p(gx), p(ws), n, st) == E
    assert lib.ps_gather_bwd(p(rptr), p(slots), N, T, p(w), null, p(g), B, H, p(gx), p(ws), n - 1, st) == E    # short workspace
    assert lib.ps_gather_bwd(p(rptr), p(slots), N, 2 ** 30, p(w), null, p(g), B, H, p(gx), p(ws), n, st) == E  # B T >= 2^31
    assert lib.ps_gather_max_arg(p(x), N, H, p(ids), p(nvalid), B, T, p(gx), null, st) == E
    assert lib.ps_gather_max_arg(p(x), N, 0, p(ids), p(nvalid), B, T, p(gx), p(arg), st) == E
    assert lib.ps_attention_bwd_rows(p(x), N, H, p(u), p(v), H, p(w2), p(ids), p(nvalid), p(w), p(g), B, T, p(w), p(gx), null,
                                     p(wr), nr, st) == E
    assert lib.ps_attention_bwd_rows(p(x), N, H, p(u), p(v), H, p(w2), p(ids), p(nvalid), p(w), p(g), B, T, p(w), p(gx), p(w2),
                                     p(wr), nr - 1, st) == E
    assert lib.ps_attention_bwd_cols(p(rptr), p(slots), N, T, p(w), p(u), p(v), 0, p(w2), B, p(gx), p(ws), n, st) == E
    assert lib.ps_attention_bwd_cols(p(rptr), p(slots), N, T, p(w), p(u), null, H, p(w2), B, p(gx), p(ws), n, st) == E
    torch.cuda.synchronize()
    assert torch.isnan(gx).all() and torch.isnan(w).all()         # a refused call writes nothing


def test_empty_problems():
    from pinsage_hip import native as nv
    from pinsage_hip import sampling
    lib = nv.lib()
    st, null = nv.stream(), nv.ptr(None)
    assert lib.ps_pool_weights(null, null, null, null, 0, 4, 9, 1, 16, null, st) == nv.PS_OK
    assert lib.ps_gather_bwd(null, null, 0, 4, null, null, null, 5, 8, null, null, 0, st) == nv.PS_OK
    assert lib.ps_gather_max_arg(null, 7, 8, null, null, 0, 4, null, null, st) == nv.PS_OK
    assert lib.ps_attention_bwd_rows(null, 7, 8, null, null, 8, null, null, null, null, null, 0, 4, null, null, null, null, 0,
                                     st) == nv.PS_OK
    assert lib.ps_attention_bwd_cols(null, null, 0, 4, null, null, null, 8, null, 5, null, null, 0, st) == nv.PS_OK
    # an empty batch through the Functions: empty outputs, zero gradients of the right shapes
    c = bc.case(0)
    x = _dev(c["x"]).requires_grad_(True)
    v = _dev(c["v"]).requires_grad_(True)
    w2 = _dev(c["w2"]).requires_grad_(True)
    u = torch.zeros((0, c["H"]), device="cuda", requires_grad=True)
    b2 = torch.zeros(1, device="cuda", requires_grad=True)
    ids = torch.empty((0, 4), dtype=torch.int32, device="cuda")
    nvalid = torch.empty(0, dtype=torch.int32, device="cuda")
    out = sampling.attention(x, u, v, w2, b2, ids, nvalid)
    assert out.shape == (0, c["H"])
    (out.sum() + sampling.max_pool(x, ids, nvalid).sum() + sampling.pool(x, ids=ids, wts=torch.empty((0, 4), device="cuda"),
                                                                         nvalid=nvalid, renorm=False).sum()).backward()
    for t in (x, v, w2, u, b2):
        assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any()
