"""tests/helpers/linear_bwd_cases.py on the CPU: the exact restatements of ps_linear_wgrad and ps_linear_epilogue_bwd against their
float64 closed forms and against torch float64 autograd of the layer they differentiate,
F.normalize(F.relu(F.linear(x, W, b) + F.linear(x2, W2))), the planted data, and the partition rule.

Bounds (derived in the helper's docstring; u = 2^-24, gamma_n = n u / (1 - n u)):
  wgrad / bias gradient   gamma_{r+p-1} sum_m |g x| for a longest chain of r = min(P, M) rows and p = ceil(M / P) partitions;
  epilogue                two reductions of lane chains of length L (+ six levels of the wave sum) and two roundings each for y and
                          the quotient: linear_bwd_cases.epilogue_bound;
  layer against autograd  the above plus what the fp32 pre-activation's own error gamma_{K+K2+1} (sum |x W| + |b|) moves the
                          epilogue's gradient by, at most 3 |G|_2 |et|_2 / c^2 per element of a row: layer_grad_bounds.
The restatements are run with small partition sizes as well: they take P as an argument, and a chain of eight rows goes wrong
in the same ways as one of 512."""
import numpy as np
import pytest

from helpers import linear_bwd_cases as lb

SMALL_P = 8


@pytest.mark.parametrize("N,K", [(1, 1), (5, 3), (33, 31)])
@pytest.mark.parametrize("M", [0, 1, 2, 7, 8, 9, 19, 64])
def test_wgrad_restatement_within_its_bound(M, N, K):
    g, x = lb.wgrad_data(M, N, K, SMALL_P)
    dW, db = lb.wgrad_exact(g, x, SMALL_P), lb.bias_grad_exact(g, SMALL_P)
    assert dW.shape == (N, K) and dW.dtype == np.float32 and db.shape == (N,)
    ref, _ = lb.wgrad_64(g, x)
    assert lb.outside(dW, ref, lb.wgrad_bound(g, x, SMALL_P)) == []
    ones = np.ones((M, 1), np.float32)
    assert lb.outside(db[:, None], lb.wgrad_64(g, ones)[0], lb.wgrad_bound(g, ones, SMALL_P)) == []
    # the bias gradient is the weight gradient against a column of ones, bit for bit
    assert lb.mismatches(db[:, None], lb.wgrad_exact(g, ones, SMALL_P)) == []
    if M == 0:
        assert not dW.view(np.uint32).any() and not db.view(np.uint32).any()


def test_wgrad_restatement_at_the_library_partition():
    P = lb.PART
    M, N, K = 2 * P + 3, 5, 3
    g, x = lb.wgrad_data(M, N, K, P)
    assert lb.outside(lb.wgrad_exact(g, x, P), lb.wgrad_64(g, x)[0], lb.wgrad_bound(g, x, P)) == []


@pytest.mark.parametrize("M,P", [(SMALL_P + 2, SMALL_P), (2 * SMALL_P + 3, SMALL_P), (5 * SMALL_P, SMALL_P),
                                 (lb.PART + 2, lb.PART), (2 * lb.PART + 3, lb.PART), (lb.doubling_rows(), 2 * lb.PART)])
def test_the_plant_tells_the_partitions_apart(M, P):
    """the planted element of dW and of db comes out different with partitions of P - 1, P + 1 or 2 P rows and as one single
    chain -- at the small sizes and at the row counts the GPU test runs"""
    N, K = 5, 3
    g, x = lb.wgrad_data(M, N, K, P)
    n, k = N // 2, K // 2
    assert (x[:, k] == 1).all() and tuple(g[P - 1:P + 2, n]) == lb.PLANT
    assert sorted(set(lb.wrong_partitions(M, P))) == sorted({P - 1, P + 1, 2 * P, M})
    want = lb.wgrad_exact(g[:, n:n + 1], x[:, k:k + 1], P)[0, 0]
    assert want == lb.plant_value(g[:, n], P) == lb.bias_grad_exact(g, P)[n]
    for other in lb.wrong_partitions(M, P):
        assert lb.wgrad_exact(g[:, n:n + 1], x[:, k:k + 1], other)[0, 0] != want, other


def test_partition_rule():
    P0, cap = lb.PART, lb.MAX_PARTS
    assert (P0, cap) == (512, 256)
    for M, P in ((0, P0), (1, P0), (P0, P0), (P0 * cap, P0), (P0 * cap + 1, 2 * P0), (2 * P0 * cap, 2 * P0),
                 (2 * P0 * cap + 1, 4 * P0), (59047, P0), (12_500_000, 65536)):
        assert lb.partition_rule(M) == P, M
        assert lb.partition(M) == P, M                                   # the library's own answer
        assert -(-M // P) <= cap
    assert lb.doubling_rows() == P0 * cap + 1
    from pinsage_hip import native
    ws = native.lib().ps_linear_wgrad_workspace_bytes
    assert ws(P0, 33, 31) == 0 and ws(0, 33, 31) == 0 and ws(P0 + 1, 0, 31) == 0 and ws(P0 + 1, 33, 0) == 0
    assert ws(P0 + 1, 33, 31) >= 2 * (33 * 31 + 33) * 4
    assert ws(12_500_000, 256, 256) <= 256 + cap * (256 * 256 + 256) * 4


@pytest.mark.parametrize("relu,l2", lb.FLAGSETS)
@pytest.mark.parametrize("N,vec", [(N, vec) for N in lb.EPILOGUE_N for vec in (1, 4) if vec == 1 or N % 4 == 0])
def test_epilogue_restatement_within_its_bound(N, vec, relu, l2):
    t, g, rows = lb.epilogue_data(N)
    gz = lb.epilogue_bwd_exact(t, g, relu, l2, vec)
    keep = lb.plain_rows(rows, t.shape[0])
    ok = keep[np.sqrt((t[keep].astype(np.float64) ** 2).sum(axis=1)) > 1e-3] if l2 else keep
    assert len(ok) >= 2
    assert lb.outside(gz[ok], lb.epilogue_bwd_64(t[ok], g[ok], relu, l2), lb.epilogue_bound(t[ok], g[ok], relu, l2, vec)) == []
    if not l2:
        want = np.where(t > 0, g, np.float32(0)) if relu else g
        assert lb.mismatches(gz, want.astype(np.float32)) == []


@pytest.mark.parametrize("N", [4, 65, 300])
def test_epilogue_planted_rows(N):
    t, g, rows = lb.epilogue_data(N)
    vec = lb.vec_of(N)
    z, a, b, n = (rows[k] for k in ("zero_row", "above_row", "below_row", "nan_row"))
    full = lb.epilogue_bwd_exact(t, g, True, True, vec)
    assert not full[z].view(np.uint32).any()                             # g / 1e-12 masked by the ReLU: +0 bits
    nomask = lb.epilogue_bwd_exact(t, g, False, True, vec)
    assert lb.mismatches(nomask[z], (g[z] / lb.CLAMP).astype(np.float32)) == []
    # just below the clamp: g / 1e-12, no projection; just above: the projection removes the component along the one entry
    assert lb.mismatches(nomask[b], (g[b] / lb.CLAMP).astype(np.float32)) == []
    assert nomask[a, N - 1] == 0 and (N == 1 or lb.mismatches(nomask[a, :N - 1], (g[a, :N - 1] / np.float32(2.0 ** -39)).astype(np.float32)) == [])
    # a NaN in t: its row is NaN (under the ReLU: wherever t > 0), no other row changes
    assert np.isnan(nomask[n]).all()
    assert (np.isnan(full[n]) == (t[n] > 0)).all() and not full[n][~(t[n] > 0)].view(np.uint32).any()
    clean = np.array(t)
    clean[n, N - 1] = 1.0
    other = lb.epilogue_bwd_exact(clean, g, False, True, vec)
    rest = [r for r in range(t.shape[0]) if r != n]
    assert lb.mismatches(nomask[rest], other[rest]) == [] and not np.isnan(nomask[rest]).any()


@pytest.mark.parametrize("relu,l2", lb.FLAGSETS)
@pytest.mark.parametrize("M,K,N,K2,bias", [(40, 16, 12, 8, True), (19, 5, 7, 0, False)])
def test_layer_restatement_against_float64_autograd(M, K, N, K2, bias, relu, l2):
    d = lb.layer_data(M, K, N, K2, bias)
    P = SMALL_P
    got = lb.layer_exact(d["x"], d["W"], d["b"], d["x2"], d["W2"], d["G"], relu, l2, P)
    bounds, ref = lb.layer_grad_bounds(d["x"], d["W"], d["b"], d["x2"], d["W2"], d["G"], relu, l2, P)
    assert np.abs(ref["t"] if not relu else ref["t"][ref["t"] > 0]).min() > 1e-4
    leaves = [k for k in ("x", "W", "b", "x2", "W2") if d[k] is not None]
    assert sorted(bounds) == sorted(leaves)
    for k in leaves:
        assert lb.outside(got[k], ref[k], bounds[k]) == [], k

