"""AttentionAggregator / MaxPoolingAggregator on their HIP kernels (csrc/neigh_agg.hip: ps_attention_weights, ps_gather_max) over
the case table of tests/helpers/agg_cases.py, against its float64 restatement of the reference, the reference's recorded outputs
(reference_golden_agg.npz) and, for the max-pool, the C oracle bit for bit -- never another GPU run.  Float results are held to
rtol 1e-5 / atol 2e-6 (tests/test_hip_model.py's embedding tolerance), maxima to equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import agg_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = ac.RTOL, ac.ATOL
NCASES = len(ac.CASES)
CASE_IDS = [f"{ci}-B{c[0]}-N{c[1]}-C{c[2]}-T{c[3]}" for ci, c in enumerate(ac.CASES)]


@pytest.fixture(scope="module")
def golden_agg():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_golden_agg.npz"))


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


def _off(ci):
    return 1 if ci == ac.OFFSET_CASE else 0


def _golden_lists(g):
    return [[int(t) for t in g["ids"][i, :g["nvalid"][i]]] for i in range(g["ids"].shape[0])]


def _load(module, g, prefix):
    sd = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
    assert set(sd) == set(module.state_dict())
    module.load_state_dict(sd)
    return module.cuda().eval()


@pytest.mark.parametrize("ci", range(NCASES), ids=CASE_IDS)
def test_attention_weights(ci):
    from pinsage_hip import sampling
    c = ac.case(ci)
    o = _off(ci)
    u, v, ids, nvalid = _dev(c["u"], o), _dev(c["v"], o), _dev(c["raw_ids"]), _dev(c["nvalid"])
    keep = ac.kept(c["raw_ids"], c["nvalid"], c["N"])
    for scale in ((1.0, 8.0) if ci == ac.SCALED_CASE else (1.0,)):
        w2 = c["w2"] * np.float32(scale)
        got = sampling.attention_weights(u, v, _dev(w2, o), ids, nvalid).cpu().numpy()
        ref = ac.attention_weights_ref(c["u"], c["v"], w2, c["raw_ids"], c["nvalid"])
        print(f"case {ci} x{scale}: max |attn - ref| {np.abs(got - ref).max():.2e}")
        assert got.shape == ref.shape and got.dtype == np.float32
        assert not got[~keep].any() and not np.signbit(got[~keep]).any()           # exactly +0.0 where nothing is kept
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
        rows = keep.any(axis=1)
        np.testing.assert_allclose(got.astype(np.float64).sum(axis=1)[rows], 1.0, rtol=0, atol=1e-6)
        single = keep.sum(axis=1) == 1
        assert single.any() and (got[single].max(axis=1) == 1.0).all()              # one neighbour: its weight is exactly 1


@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_attention_softmax_is_stable(sign):
    """scores of magnitude > 80 with one neighbour more than 100 above the rest: exp() of a raw score or of a raw difference
    would overflow / underflow to 0 / 0"""
    from pinsage_hip import sampling
    B, N, Hd, T, P = 8, 32, 64, 12, 5
    rs = np.random.RandomState(3)
    lo, hi = (1.0, 3.0) if sign > 0 else (3.0, 1.0)         # relu(1 + v) summed over 64 columns: 128 and 256 (sign -1: -256 and -128)
    v = (lo + 0.01 * rs.standard_normal((N, Hd))).astype(np.float32)
    v[P] = hi
    u = np.ones((B, Hd), dtype=np.float32)
    w2 = np.full(Hd, sign, dtype=np.float32)
    ids = rs.randint(0, N - 1, size=(B, T)).astype(np.int32)
    ids[ids == P] = N - 1
    ids[np.arange(B), np.arange(B) % T] = P                 # the planted neighbour, once per row
    nvalid = np.full(B, T, dtype=np.int32)
    s = ac.attention_weights_ref(u, v, w2, ids, nvalid)     # float64 scores behind it:
    sc = np.maximum(u[:, None, :].astype(np.float64) + v[ids], 0.0) @ w2.astype(np.float64)
    assert (np.abs(sc) > 80).all()
    planted = ids == P
    assert (sc[planted][:, None] - sc[~planted].reshape(B, T - 1) > 100).all()
    got = sampling.attention_weights(_dev(u), _dev(v), _dev(w2), _dev(ids), _dev(nvalid)).cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got[planted], 1.0, rtol=0, atol=1e-6)
    np.testing.assert_allclose(got, s, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("ci", range(NCASES), ids=CASE_IDS)
def test_attention_aggregator(ci):
    c = ac.case(ci)
    x, sx = _dev(c["x"], _off(ci)), _dev(c["self_x"], _off(ci))
    for scaled in ((False, True) if ci == ac.SCALED_CASE else (False,)):
        at, _ = ac.modules(ci, scaled)
        ref = ac.at_ref(at, c["x"], c["neighbors"], c["self_x"])
        ref_self = ac.at_ref(at, c["x"], c["neighbors"]) if c["N"] >= c["B"] else None
        at.cuda()
        with torch.no_grad():
            got = at(x, c["neighbors"], sx).cpu().numpy()
            print(f"case {ci} scaled {scaled}: max |out - ref| {np.abs(got - ref).max():.2e}")
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
            assert not got[c["nvalid"] == 0].any()
            if ref_self is not None:                          # self_features = None: the first B rows of `features`
                np.testing.assert_allclose(at(x, c["neighbors"]).cpu().numpy(), ref_self, rtol=RTOL, atol=ATOL)


def test_attention_aggregator_golden(golden_agg):
    from model import aggregators as A
    a = golden_agg
    at = _load(A.AttentionAggregator(64), a, "at_")
    with torch.no_grad():
        got = at(_dev(a["features"]), _golden_lists(a), _dev(a["self_features"])).cpu().numpy()
    np.testing.assert_allclose(got, a["attention"], rtol=RTOL, atol=ATOL)
    assert not got[a["nvalid"] == 0].any()


@pytest.mark.parametrize("ci", range(NCASES), ids=CASE_IDS)
def test_gather_max(ci):
    from pinsage_hip import sampling
    c = ac.case(ci)
    o = _off(ci)
    ids, nvalid = _dev(c["raw_ids"]), _dev(c["nvalid"])
    x = -np.abs(c["x"]) - 1.0                               # all negative: a maximum started from 0 would show
    got = sampling.gather_max(_dev(x, o), ids, nvalid).cpu().numpy()
    ref = ac.gather_max_ref(x, c["raw_ids"], c["nvalid"])
    assert np.array_equal(got, ref) and not np.signbit(got[ref == 0]).any()
    keep = ac.kept(c["raw_ids"], c["nvalid"], c["N"])
    assert (ref[keep.any(axis=1)] < 0).all() and not ref[~keep.any(axis=1)].any()
    x = x.copy()
    i, j = np.argwhere(keep)[-1]
    x[c["raw_ids"][i, j], 0] = np.nan                       # a gathered NaN
    if c["C"] > 1:
        x[:, c["C"] - 1] = -np.inf                          # a column whose maximum is -inf
    got = sampling.gather_max(_dev(x, o), ids, nvalid).cpu().numpy()
    ref = ac.gather_max_ref(x, c["raw_ids"], c["nvalid"])
    assert np.isnan(ref[i, 0]) and (c["C"] == 1 or np.isneginf(ref[i, -1]))
    assert np.array_equal(got, ref, equal_nan=True)


@pytest.mark.parametrize("ci", range(NCASES), ids=CASE_IDS)
def test_maxpool_aggregator(ci):
    """ps_linear is bit-exact to the oracle's linear and a maximum has no order: equality"""
    from oracle import c_oracle as co
    c = ac.case(ci)
    _, mp = ac.modules(ci)
    p = {k: t.detach().numpy() for k, t in mp.state_dict().items()}
    t = co.linear(c["x"], p["mlp.0.weight"], p["mlp.0.bias"], relu=True)
    ref = ac.gather_max_ref(t, c["ids"], c["nvalid"])
    np.testing.assert_allclose(ref, ac.mp_ref(mp, c["x"], c["neighbors"]), rtol=RTOL, atol=ATOL)      # the oracle chain is the formula
    mp.cuda()
    with torch.no_grad():
        got = mp(_dev(c["x"], _off(ci)), c["neighbors"]).cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got, ref)


def test_maxpool_aggregator_golden(golden_agg):
    from model import aggregators as A
    a = golden_agg
    mp = _load(A.MaxPoolingAggregator(64, 48), a, "mp_")
    with torch.no_grad():
        got = mp(_dev(a["features"]), _golden_lists(a)).cpu().numpy()
    np.testing.assert_allclose(got, a["maxpool"], rtol=RTOL, atol=ATOL)
    assert not got[a["nvalid"] == 0].any()


def test_attention_builds_no_padded_float_tensor():
    """B = N = 4096, C = 64, T = 32: the HIP path's peak allocation stays below ONE [B, T, C] fp32 tensor (its own tensors -- u, v,
    attn, out, ids, nvalid -- are about 4 (3 B C + 3 B T) bytes: 5 MB against 33 MB); the torch path builds at least two"""
    from model import aggregators as A
    B = N = 4096
    C, T = 64, 32
    rs = np.random.RandomState(11)
    x = _dev(rs.standard_normal((N, C)).astype(np.float32))
    nb = rs.randint(0, N, size=(B, T)).tolist()
    torch.manual_seed(5)
    at = A.AttentionAggregator(C).cuda().eval()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = fn(x, nb)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    grew, out = peak(at)
    grew_torch, out_torch = peak(at._forward_torch)
    print(f"peak allocation: HIP path {grew} bytes, torch path {grew_torch} bytes; one [B,T,C] tensor {4 * B * T * C}")
    assert grew < 4 * B * T * C
    assert grew_torch >= 8 * B * T * C
    np.testing.assert_allclose(out.cpu().numpy(), out_torch.cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_empty_batch():
    """no neighbour lists at all: an empty [0, C] / [0, out] result, as the torch code gives (an empty tensor's base is NULL)"""
    from pinsage_hip import sampling
    c = ac.case(3)
    at, mp = ac.modules(3)
    at.cuda(), mp.cuda()
    x = _dev(c["x"])
    with torch.no_grad():
        a, m = at(x, []), mp(x, [])
        assert a.shape == (0, c["C"]) and m.shape == (0, ac.out_channels(3)) and a.is_cuda and m.is_cuda
        assert a.shape == at._forward_torch(x, []).shape and m.shape == mp._forward_torch(x, []).shape
        a = at(x, [], _dev(c["self_x"]))
        assert a.shape == (0, c["C"])
    ids = torch.empty((0, 4), dtype=torch.int32, device="cuda")
    nvalid = torch.empty(0, dtype=torch.int32, device="cuda")
    assert sampling.attention_weights(x[:0], x, x[0], ids, nvalid).shape == (0, 4)
    assert sampling.gather_max(x, ids, nvalid).shape == (0, c["C"])


def test_dispatch():
    """autograd sees the call -> the torch path (same forward within tolerance, gradients arrive); otherwise the kernels, and
    they give the same bits on every run"""
    c = ac.case(3)
    at, mp = ac.modules(3)
    at.cuda(), mp.cuda()
    x, sx = _dev(c["x"]), _dev(c["self_x"])
    with torch.no_grad():
        a0, m0 = at(x, c["neighbors"], sx), mp(x, c["neighbors"])
        a1, m1 = at(x, c["neighbors"], sx), mp(x, c["neighbors"])
    assert not a0.requires_grad and not m0.requires_grad
    assert np.array_equal(a0.cpu().numpy(), a1.cpu().numpy()) and np.array_equal(m0.cpu().numpy(), m1.cpu().numpy())
    xg = x.clone().requires_grad_(True)
    ag, mg = at(xg, c["neighbors"], sx), mp(xg, c["neighbors"])          # parameters require grad, grad mode on
    assert ag.requires_grad and mg.requires_grad
    np.testing.assert_allclose(ag.detach().cpu().numpy(), a0.cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(mg.detach().cpu().numpy(), m0.cpu().numpy(), rtol=RTOL, atol=ATOL)
    (ag.sum() + mg.sum()).backward()
    assert at.attention[0].weight.grad is not None and at.attention[0].weight.grad.abs().sum() > 0
    assert mp.mlp[0].weight.grad is not None and xg.grad is not None and xg.grad.abs().sum() > 0
    # frozen parameters and plain features: the kernels, with grad mode on
    for p in list(at.parameters()) + list(mp.parameters()):
        p.requires_grad_(False)
    assert np.array_equal(at(x, c["neighbors"], sx).cpu().numpy(), a0.cpu().numpy())
    assert np.array_equal(mp(x, c["neighbors"]).cpu().numpy(), m0.cpu().numpy())
    # fp64 features: the torch path, as before
    at.double()
    out = at(x.double(), c["neighbors"], sx.double())
    assert out.dtype == torch.float64
    np.testing.assert_allclose(out.cpu().numpy(), a0.cpu().numpy(), rtol=RTOL, atol=ATOL)
