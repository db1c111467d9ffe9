"""The restatement of the neighbour-gather backward kernels (tests/helpers/agg_bwd_cases.py) is itself checked here, without a
GPU: against float64 closed-form gradients within derived bounds, and against torch CPU autograd of the modules' `_torch_padded`
expressions on a seed where no ReLU or arg-max decision can flip between the two roundings."""
import numpy as np
import pytest
import torch

from helpers import agg_bwd_cases as bc
from helpers import agg_cases as ac

GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-5           # tests/test_hip_model.py's gradient tolerance
CPU_CASES = (0, 1, 2, 3, 5, bc.HUB_CASE, bc.HUB_CASE + 1)


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} entries beyond the bound, worst {err[bad].max()} against {bound[bad].min()}"


def test_case_table_plants_what_it_says():
    seg = bc.segment()
    assert seg >= 8
    seen_vec, seen_T = set(), set()
    for ci in range(len(bc.CASES)):
        c = bc.case(ci)
        seen_vec.add(c["vec"])
        seen_T.add(c["T"])
        if c["B"] != 50:
            continue
        keep = ac.kept(c["ids"], c["nvalid"], c["N"])
        rptr, _ = bc.slot_lists_ref(c["ids"], keep, c["N"])
        assert list(np.diff(rptr)[90:95]) == [0, 1, 7, 8, 9]
        assert c["nvalid"][7] == 0 and c["nvalid"][8] > c["T"] and c["nvalid"][9] < 0
        assert (c["x"][80:84] < 0).all() and np.array_equal(c["x"][84], c["x"][85])
        if c["T"] >= 3:
            assert len(set(c["ids"][3, :3])) == 1 and c["ids"][5, 0] == -1 and c["ids"][5, 1] == c["N"] and c["ids"][5, 2] > c["max_idx"]
        if c["T"] >= 2:
            _, arg = bc.gather_max_arg_ref(c["x"], c["ids"], c["nvalid"])
            assert (arg[13] == 0).all()                           # the tie goes to the lower slot
    assert seen_vec == {1, 4} and {1, 10, 16, 17, 70} <= seen_T
    a, b = bc.case(bc.HUB_CASE), bc.case(bc.HUB_CASE + 1)
    assert a["B"] == b["B"] == 2 * seg + 3 and a["T"] == b["T"] == 2
    na = np.diff(bc.slot_lists_ref(a["ids"], ac.kept(a["ids"], a["nvalid"], a["N"]), a["N"])[0])
    nb = np.diff(bc.slot_lists_ref(b["ids"], ac.kept(b["ids"], b["nvalid"], b["N"]), b["N"])[0])
    assert na[0] == seg - 1 and na[2] == seg + 1 and na[3] == 2 * seg + 3 and nb[1] == seg and nb[3] == 2 * seg + 3


@pytest.mark.parametrize("ci", CPU_CASES)
def test_gather_bwd_restatement_against_float64(ci):
    c = bc.case(ci)
    B, N, T = c["B"], c["N"], c["T"]
    seg = bc.segment()
    for use_counts, renorm in ((True, True), (False, False)):
        w = bc.pool_weights_exact(c["ids"], c["counts"] if use_counts else None, None if use_counts else c["wts"], c["nvalid"],
                                  c["max_idx"], renorm, 16)
        keep = bc.kept_pool(c["ids"], c["nvalid"], c["max_idx"])
        assert not w[~keep].any() and not np.signbit(w[~keep]).any()
        if renorm:                                                # renormalised weights sum to one within T roundings
            rows = keep.any(axis=1)
            assert np.abs(w.astype(np.float64).sum(axis=1)[rows] - 1.0).max() <= (T + 2) * bc.U32
        rptr, slots = bc.slot_lists_ref(c["ids"], keep, N)
        got = bc.gather_bwd_exact(rptr, slots, N, T, c["g"], coef=w)
        want, mag = bc.gather_bwd_64(c["ids"], keep, N, c["g"], w)
        n = np.diff(rptr)
        _within(got, want, bc.chain_bound((n + np.ceil(n / seg))[:, None], mag), f"case {ci} pool gx")
        assert not got[n == 0].any()
    # max: every kept (row, column) hands its gradient to exactly one slot
    keep = ac.kept(c["ids"], c["nvalid"], N)
    out, arg = bc.gather_max_arg_ref(c["x"], c["ids"], c["nvalid"])
    assert np.array_equal(out, ac.gather_max_ref(c["x"], c["ids"], c["nvalid"]))
    rptr, slots = bc.slot_lists_ref(c["ids"], keep, N)
    got = bc.gather_bwd_exact(rptr, slots, N, T, c["g"], arg=arg)
    want, mag = np.zeros((N, c["H"])), np.zeros((N, c["H"]))
    cnt = np.zeros((N, c["H"]))
    for i in range(B):
        if keep[i].any():
            rows = c["ids"][i, arg[i]]
            np.add.at(want, (rows, np.arange(c["H"])), c["g"][i].astype(np.float64))
            np.add.at(mag, (rows, np.arange(c["H"])), np.abs(c["g"][i].astype(np.float64)))
            np.add.at(cnt, (rows, np.arange(c["H"])), 1.0)
            assert np.array_equal(c["x"][rows, np.arange(c["H"])], out[i])
    _within(got, want, bc.chain_bound(cnt + np.ceil(cnt / seg), mag), f"case {ci} max gx")


@pytest.mark.parametrize("ci", CPU_CASES)
def test_attention_restatement_against_float64(ci):
    c = bc.case(ci)
    N, T = c["N"], c["T"]
    keep = ac.kept(c["ids"], c["nvalid"], N)
    scores = ac.attention_scores_exact(c["u"], c["v"], c["w2"], c["ids"], c["nvalid"], c["vec"])
    attn = ac.softmax_of_scores(scores).astype(np.float32)       # a forward result in fp32: the backward's input
    ds, du, dw2, _ = bc.attention_bwd_rows_exact(c["x"], c["u"], c["v"], c["w2"], c["ids"], c["nvalid"], attn, c["g"], c["vec"])
    rptr, slots = bc.slot_lists_ref(c["ids"], keep, N)
    dv = bc.attention_bwd_cols_exact(rptr, slots, N, T, ds, c["u"], c["v"], c["w2"])
    bnd, val = bc.attention_bounds(c["x"], c["u"], c["v"], c["w2"], c["ids"], c["nvalid"], attn, c["g"])
    assert not ds[~keep].any()
    for name, got in (("ds", ds), ("du", du), ("dw2", dw2)):
        _within(got, val[name], bnd[name], f"case {ci} {name}")
    # dv chains the fp32 ds: centre the check on float64 sums of those, with the chain's own bound on top of ds's error
    _within(dv, val["dv"], bnd["dv"], f"case {ci} dv")
    dx = bc.gather_bwd_exact(rptr, slots, N, T, c["g"], coef=attn)
    want, mag = bc.gather_bwd_64(c["ids"], keep, N, c["g"], attn)
    n = np.diff(rptr)
    _within(dx, want, bc.chain_bound((n + np.ceil(n / bc.segment()))[:, None], mag), f"case {ci} attention dx")


def _autograd_case(seed):
    """small module-shaped inputs: (features [N,C], self [B,C], ids, nvalid) with legal ids and -1 padding"""
    rs = np.random.RandomState(seed)
    B, N, C, T = 23, 40, 12, 6
    x = rs.standard_normal((N, C)).astype(np.float32)
    sx = rs.standard_normal((B, C)).astype(np.float32)
    nvalid = rs.randint(0, T + 1, size=B).astype(np.int32)
    nvalid[:3] = [T, 0, 1]
    ids = rs.randint(0, N, size=(B, T)).astype(np.int32)
    ids[4, 1] = ids[4, 0]
    ids[np.arange(T)[None, :] >= nvalid[:, None]] = -1
    return B, N, C, T, x, sx, ids, nvalid


SEED = 3


def test_attention_restatement_against_torch_autograd():
    from model import aggregators as A
    B, N, C, T, x, sx, ids, nvalid = _autograd_case(SEED)
    torch.manual_seed(100 + SEED)
    at = A.AttentionAggregator(C)
    W1, b1 = at.attention[0].weight.detach().numpy(), at.attention[0].bias.detach().numpy()
    w2 = at.attention[2].weight.detach().numpy().reshape(-1)
    u64 = sx.astype(np.float64) @ W1[:, :C].astype(np.float64).T + b1
    v64 = x.astype(np.float64) @ W1[:, C:].astype(np.float64).T
    rs = np.random.RandomState(50 + SEED)
    g = rs.standard_normal((B, C)).astype(np.float32)
    ref64 = bc.attention_grads_64(x, u64, v64, w2, ids, nvalid, g)
    assert ref64["hmin"] > 1e-4, ref64["hmin"]                    # no ReLU decision can flip between roundings
    xt, st = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(sx).requires_grad_(True)
    out = at._torch_padded(xt, torch.from_numpy(ids), torch.from_numpy(nvalid), st)
    out.backward(torch.from_numpy(g))
    # the restatement on fp32 u, v as F.linear makes them, chained back through the linears in float64
    u = (sx @ W1[:, :C].T + b1).astype(np.float32)
    v = (x @ W1[:, C:].T).astype(np.float32)
    keep = ac.kept(ids, nvalid, N)
    attn = ac.softmax_of_scores(ac.attention_scores_exact(u, v, w2, ids, nvalid, 4)).astype(np.float32)
    ds, du, dw2, _ = bc.attention_bwd_rows_exact(x, u, v, w2, ids, nvalid, attn, g, 4)
    rptr, slots = bc.slot_lists_ref(ids, keep, N)
    dv = bc.attention_bwd_cols_exact(rptr, slots, N, T, ds, u, v, w2)
    dx = bc.gather_bwd_exact(rptr, slots, N, T, g, coef=attn)
    W1d = W1.astype(np.float64)
    dx_total = dx + dv.astype(np.float64) @ W1d[:, C:]
    dsx = du.astype(np.float64) @ W1d[:, :C]
    dW1 = np.concatenate([du.astype(np.float64).T @ sx, dv.astype(np.float64).T @ x], axis=1)
    tol = dict(rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(dx_total, xt.grad.numpy(), **tol)
    np.testing.assert_allclose(dsx, st.grad.numpy(), **tol)
    np.testing.assert_allclose(dW1, at.attention[0].weight.grad.numpy(), **tol)
    np.testing.assert_allclose(du.astype(np.float64).sum(axis=0), at.attention[0].bias.grad.numpy(), **tol)
    np.testing.assert_allclose(dw2, at.attention[2].weight.grad.numpy().reshape(-1), **tol)
    assert not at.attention[2].bias.grad.abs().max() > 1e-6       # the bias drops out of the softmax


def test_max_restatement_against_torch_autograd():
    from model import aggregators as A
    B, N, C, T, x, _, ids, nvalid = _autograd_case(SEED)
    torch.manual_seed(200 + SEED)
    mp = A.MaxPoolingAggregator(C, 10)
    W, b = mp.mlp[0].weight.detach().numpy(), mp.mlp[0].bias.detach().numpy()
    pre64 = x.astype(np.float64) @ W.astype(np.float64).T + b
    assert np.abs(pre64).min() > 1e-4                             # no ReLU decision can flip between roundings
    t64 = np.maximum(pre64, 0.0)
    keep = ac.kept(ids, nvalid, N)
    # no ties: within every kept list (duplicates of one id aside) the float64 maximum is attained by one id -- or it is the
    # ReLU's exact zero, which passes no gradient whichever slot holds it
    for i in range(B):
        js = np.nonzero(keep[i])[0]
        if js.size > 1:
            rows = t64[np.unique(ids[i, js])]
            top = np.sort(rows, axis=0)
            assert rows.shape[0] == 1 or ((top[-1] - top[-2] > 1e-4) | (top[-1] == 0)).all(), i
    rs = np.random.RandomState(60 + SEED)
    g = rs.standard_normal((B, 10)).astype(np.float32)
    xt = torch.from_numpy(x).requires_grad_(True)
    out = mp._torch_padded(xt, torch.from_numpy(ids), torch.from_numpy(nvalid))
    out.backward(torch.from_numpy(g))
    t = np.maximum((x @ W.T + b).astype(np.float32), np.float32(0.0))
    _, arg = bc.gather_max_arg_ref(t, ids, nvalid)
    rptr, slots = bc.slot_lists_ref(ids, keep, N)
    gt = bc.gather_bwd_exact(rptr, slots, N, T, g, arg=arg).astype(np.float64) * (t > 0)
    tol = dict(rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(gt @ W.astype(np.float64), xt.grad.numpy(), **tol)
    np.testing.assert_allclose(gt.T @ x, mp.mlp[0].weight.grad.numpy(), **tol)
    np.testing.assert_allclose(gt.sum(axis=0), mp.mlp[0].bias.grad.numpy(), **tol)
