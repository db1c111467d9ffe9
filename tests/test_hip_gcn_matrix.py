"""The fused GCN layer (ps_gcn_layer: gcn_count_kernel, gcn_order_kernel, gemm_f32_kernel<1,4,2,2,32,0,true,GCN=1>) and the
neighbour pooling (ps_importance_pool: both kernels) against the C oracle -- never another GPU run.  tests/helpers/gcn_cases.py
holds the table (the class boundary planted at 0, 1, 64 j, 64 j + 1, M - 1 and M heavy rows, K != H, second pooling sweeps,
nvalid above T, two passes of the order kernel per chunk, ...) and tests/test_gcn_cases.py proves on the CPU that each case
produces its situation.  Before the norm the layer computes the oracle's bits (pool_ex's pooling fed into the fmaf chain); the
test accepts the fp64 norm of those bits within gemm_cases.norm_bound(256), rows that are zero before the norm as +0, and a NaN
that the call did not overwrite nowhere.  The pooling kernels must equal pool_ex bit for bit, each in its own summation order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gcn_cases as gn  # noqa: E402
import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCH_NAMES = ("PS_GCN_FUSED", "PS_GEMM_SHARD", "PS_GEMM_PERSIST", "PS_GEMM_DMA", "PS_POOL_ROWS_PER_WAVE")
BY_NAME = {c.name: c for c in gn.FUSED_CASES}


def _dev(a):
    return None if a is None else torch.tensor(a).cuda()                  # a copy: the cached arrays are read-only


def _operands(c):
    """x, W, b, h_full, ids, counts / wts, nvalid, W2 on the device.  c.wslice: W and W2 are views of one [256, K + H] matrix"""
    d = gn.gcn_data(c)
    counts, wts = gn.form_args(d.rows, c.form)
    x = _dev(d.x)
    h_full = x if c.h_is_x else _dev(d.h_full)
    if c.wslice:
        big = _dev(d.Wbig)
        W, W2 = big[:, :c.K], big[:, c.K:]
        assert W.stride(0) == W2.stride(0) == c.K + c.H and W2.data_ptr() - big.data_ptr() == 4 * c.K and not W2.is_contiguous()
    else:
        W, W2 = _dev(d.W), _dev(d.W2)
    return dict(x=x, W=W, b=_dev(d.b), h_full=h_full, ids=_dev(d.rows.ids), counts=_dev(counts), wts=_dev(wts),
                nvalid=_dev(d.rows.nvalid), W2=W2, max_idx=d.max_idx_arg)


def _fused(x, W, b, h_full, ids, counts, wts, nvalid, W2, max_idx, renorm):
    """ps_gcn_layer itself into a y of NaN: a row the order misses shows, and an unserved call fails here (no fall-back)"""
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    staged = isinstance(W, dense.StagedWeight)
    Wm, W2m = (W.t, W2.t) if staged else (W, W2)
    M, K = x.shape
    n_full, H = h_full.shape
    T = ids.size(1)
    L = nv.lib()
    wsb = int(L.ps_gcn_layer_workspace_bytes(nv.i64(M), nv.i32(H)))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    y = torch.full((M, Wm.size(0)), float("nan"), device=x.device)
    flags = nv.PS_RELU | nv.PS_L2NORM | (nv.PS_WPERM if staged else 0)
    rc = L.ps_gcn_layer(nv.ptr(x), nv.i64(M), nv.i32(K), nv.C.c_void_p(Wm.data_ptr()), nv.i32(Wm.stride(0)), nv.ptr(b),
                        nv.i32(Wm.size(0)), nv.ptr(h_full), nv.i64(n_full), nv.i32(H), nv.ptr(ids), nv.ptr(counts), nv.ptr(wts),
                        nv.ptr(nvalid), nv.i32(T), nv.i64(max_idx), nv.i32(renorm), nv.C.c_void_p(W2m.data_ptr()),
                        nv.i32(W2m.stride(0)), nv.i32(flags), nv.ptr(y), nv.ptr(ws), nv.C.c_size_t(wsb), nv.stream())
    assert rc == nv.PS_OK, rc
    return y


def _check(c, y, renorm, what):
    got = y.cpu().numpy()
    assert got.shape == (c.M, 256) and got.dtype == np.float32
    bad = gn.gcn_mismatches(got, c, renorm)
    print(f"{c.name} renorm={renorm} {what}: {'ok' if not bad else bad}")
    if bad:
        f = gn.facts(c)
        ord_, nheavy = gn.partition(gn.gcn_data(c).keeps)
        pos = int(np.flatnonzero(ord_ == bad[0][0])[0])
        pytest.fail(f"case {c.name} ({what}, form {c.form}, renorm {renorm}): {c.situation}.  By the restated launcher: {f}.  First "
                    f"(row, col, got, want): {bad}; row {bad[0][0]} is position {pos} of the order (tile {pos // 64}, "
                    f"{'heavy' if pos < nheavy else 'keeps nothing'}); bound {gc.norm_bound(256):.3e} relative")


@pytest.mark.parametrize("c", gn.FUSED_CASES, ids=lambda c: c.name)
def test_gcn_layer_matrix_vs_oracle(c, monkeypatch):
    from pinsage_hip import dense
    for name in SWITCH_NAMES:
        monkeypatch.delenv(name, raising=False)
    ops = _operands(c)
    for renorm in c.renorms:
        _check(c, _fused(**ops, renorm=renorm), renorm, "ps_gcn_layer")
    if c.wslice:                                                           # the same views in image order (PS_WPERM)
        staged = dict(ops, W=dense.stage_weight(ops["W"]), W2=dense.stage_weight(ops["W2"]))
        assert isinstance(staged["W"], dense.StagedWeight) and isinstance(staged["W2"], dense.StagedWeight)
        for renorm in c.renorms:
            _check(c, _fused(**staged, renorm=renorm), renorm, "ps_gcn_layer, image-order weights")
            # and through the wrapper, which must hand the views over without a copy
            y = dense.gcn_layer(ops["x"], ops["W"], ops["b"], ops["h_full"], ops["ids"], ops["counts"], ops["nvalid"], ops["W2"],
                                wts=ops["wts"], max_idx=ops["max_idx"], renorm=bool(renorm))
            _check(c, y, renorm, "dense.gcn_layer")


def _gcn_layer(ops, renorm):
    from pinsage_hip import dense
    return dense.gcn_layer(ops["x"], ops["W"], ops["b"], ops["h_full"], ops["ids"], ops["counts"], ops["nvalid"], ops["W2"],
                           wts=ops["wts"], max_idx=ops["max_idx"], renorm=bool(renorm))


@pytest.mark.parametrize("c", gn.UNSERVED_CASES, ids=lambda c: c.name)
def test_gcn_layer_unserved_shapes_vs_oracle(c, monkeypatch):
    """dense.gcn_layer where ps_gcn_layer declines (M < 24 576, T > 16): the pair ps_importance_pool + ps_linear, held to the
    same oracle"""
    from pinsage_hip import native as nv
    for name in SWITCH_NAMES:
        monkeypatch.delenv(name, raising=False)
    ops = _operands(c)
    for renorm in c.renorms:
        with pytest.raises(AssertionError, match=str(nv.PS_EUNSUPPORTED)):
            _fused(**ops, renorm=renorm)
        _check(c, _gcn_layer(ops, renorm), renorm, f"dense.gcn_layer, unserved: {c.situation}")


def test_gcn_layer_switched_off_vs_oracle(monkeypatch):
    from pinsage_hip import native as nv
    c = BY_NAME[gn.SWITCHED_OFF_CASE]
    for name in SWITCH_NAMES:
        monkeypatch.delenv(name, raising=False)
    ops = _operands(c)
    monkeypatch.setenv("PS_GCN_FUSED", "0")
    for renorm in c.renorms:
        with pytest.raises(AssertionError, match=str(nv.PS_EUNSUPPORTED)):
            _fused(**ops, renorm=renorm)
        _check(c, _gcn_layer(ops, renorm), renorm, "dense.gcn_layer under PS_GCN_FUSED=0")


@pytest.mark.parametrize("c", gn.POOL_CASES, ids=lambda c: c.name)
def test_importance_pool_matrix_vs_oracle(c, monkeypatch):
    """sampling.importance_pool, both forms, renorm 0 / 1, bit-equal to pool_ex in the launched kernel's summation order (16
    lanes: the four-rows-per-wave kernel; 64: the one-wave-per-row kernel).  At T <= 16 the other kernel is run too (by the
    switch, where H % 4 == 0): identical bits, as include/pinsage_hip.h says."""
    from pinsage_hip import sampling
    d = gn.pool_data(c)
    x, ids, nvalid = _dev(d.x), _dev(d.rows.ids), _dev(d.rows.nvalid)
    assert x.data_ptr() % 16 == 0
    for form, renorm in gn.POOL_RUNS:
        counts, wts = gn.form_args(d.rows, form)
        kw = dict(ids=ids, counts=_dev(counts), wts=_dev(wts), nvalid=nvalid, max_idx=d.max_idx, renorm=bool(renorm))
        monkeypatch.delenv("PS_POOL_ROWS_PER_WAVE", raising=False)
        for name, value in c.env:
            monkeypatch.setenv(name, value)
        got = sampling.importance_pool(x, **kw).cpu().numpy()
        want = gn.pool_ref(c, form, renorm, gn.lanes_of(c.kernel))
        bad = gc.mismatches_exact(got, want)
        print(f"{c.name} {form} renorm={renorm}: {'ok' if not bad else bad}")
        assert not bad, (f"case {c.name} ({c.kernel} kernel, {form}, renorm {renorm}): first (row, col, got, want): {bad}; "
                         f"nvalid of row {bad[0][0]}: {int(d.rows.nvalid[bad[0][0]])}, kind {int(d.rows.kind[bad[0][0]])}")
        if c.T <= 16 and c.H % 4 == 0:
            other = "four" if c.kernel == "wave" else "wave"
            if other == "wave":
                monkeypatch.setenv("PS_POOL_ROWS_PER_WAVE", "1")
            else:
                monkeypatch.delenv("PS_POOL_ROWS_PER_WAVE", raising=False)
            assert gn.pool_kernel(c.T, c.H, (("PS_POOL_ROWS_PER_WAVE", "1"),) if other == "wave" else ()) == other
            again = sampling.importance_pool(x, **kw).cpu().numpy()
            bad = gc.mismatches_exact(again, want)
            assert not bad, f"case {c.name}: the {other} kernel at T <= 16 ({form}, renorm {renorm}): {bad}"
