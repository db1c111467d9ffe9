"""The plain-C oracle (oracle/pinsage_oracle.c) against the reference's golden vectors and
against the numpy oracle on seeded random inputs.  CPU only."""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import pinsage_oracle as orc
from conftest import bipartite_graph

G1 = {"A": 3, "B": 1, "C": 2, "D": 1, "E": 1}


def _cgraph(g, name):
    ew = g[f"{name}_edge_weights"] if f"{name}_edge_weights" in g.files else None
    return co.Graph(g[f"{name}_edge_index"], ew)


def test_np_sum_bit_exact():
    rs = np.random.RandomState(1)
    for n in [0, 1, 7, 8, 9, 127, 128, 129, 1000, 8192, 8193, 9001, 20000, 81237]:
        a = rs.random_sample(n) * 5 + 0.01
        assert co.np_sum(a) == float(a.sum()), n


def test_csr_cdf_match_numpy_oracle():
    for weights in ("half", "float", None):
        ei, ew = bipartite_graph(40, 30, 600, 3, weights)
        g = co.Graph(ei, ew)
        rowptr, col, w = orc.csr_from_edges(ei, ew)
        cdf = orc.cdf_from_csr(rowptr, w)
        assert np.array_equal(g.rowptr, rowptr) and np.array_equal(g.col, col)
        assert np.array_equal(g.cdf, cdf)                      # fp64 bit-exact


@pytest.mark.parametrize("name", sorted(G1))
def test_sampler_golden(golden, name):
    g = golden
    cg = _cgraph(g, f"g1_{name}")
    rs = np.random.RandomState(int(g[f"g1_{name}_npseed"]))
    for ci in range(G1[name]):
        pre = f"g1_{name}_{ci}_"
        W, L, T = [int(v) for v in g[pre + "WLT"]]
        nodes = g[pre + "nodes"]
        uoff, n = cg.uniform_offsets(nodes, W, L)
        u = rs.random_sample(n)
        for kw in (dict(), dict(uoff=uoff, threads=4)):        # sequential and offset/parallel forms
            ids, counts, nv, wts, used, _ = co.walk_sample(cg, nodes, T, L, W, uniforms=u, **kw)
            assert np.array_equal(ids, g[pre + "ids"])
            assert np.array_equal(nv, g[pre + "nvalid"])
            assert np.array_equal(wts, g[pre + "weights"])
        assert used == 0 or used == n
    assert rs.random_sample() == float(g[f"g1_{name}_tail"])


def test_sampler_sink_golden(golden):
    g = golden
    cg = _cgraph(g, "g1_S")
    u = np.random.RandomState(7).random_sample(300)
    ids, counts, nv, wts, used, _ = co.walk_sample(cg, [0, 1, 2, 3, 4], 4, 3, 20, uniforms=u)
    assert np.array_equal(ids, g["g1_S_ids"]) and np.array_equal(wts, g["g1_S_weights"])
    rs = np.random.RandomState(7)
    rs.random_sample(used)
    assert rs.random_sample() == float(g["g1_S_tail"])


def test_single_walk_golden(golden):
    g = golden
    cg = _cgraph(g, "g6")
    u = np.random.RandomState(11).random_sample(24)
    pos = 0
    for s, ref in zip(g["g6_starts"], g["g6_walks"]):
        walk, pos = co.single_walk(cg, int(s), 4, u, pos)
        assert walk == ref.tolist()


def test_philox_matches_numpy_oracle():
    ei, ew = bipartite_graph(50, 40, 700, 5, "half")
    cg = co.Graph(ei, ew)
    rowptr, col, w = orc.csr_from_edges(ei, ew)
    cdf = orc.cdf_from_csr(rowptr, w)
    nodes = np.arange(50)
    a = co.walk_sample(cg, nodes, 10, 2, 20, philox=(0x1234567890ABCDEF, 3), threads=3)
    b = orc.batch_sample_neighbors(rowptr, col, cdf, nodes, 10, 2, 20, philox=(0x1234567890ABCDEF, 3))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


def test_pool_and_forward_golden(golden):
    from test_oracle_golden import _counts_from_weights
    g = golden
    counts = _counts_from_weights(g["g2_weights"], g["g2_nvalid"])
    for tag in ("items", "all"):
        out = co.importance_pool(g[f"g2_h_{tag}"], g["g2_ids"], counts, g["g2_nvalid"])
        np.testing.assert_allclose(out, g[f"g2_out_{tag}"], rtol=1e-5, atol=1e-6)
    params = {k[len("g3_param_"):]: g[k] for k in g.files if k.startswith("g3_param_")}
    layers = []
    for li in range(2):
        nv = g[f"g3_l{li}_nvalid"]
        layers.append((g[f"g3_l{li}_ids"], _counts_from_weights(g[f"g3_l{li}_weights"], nv), nv))
    np.testing.assert_allclose(co.pinsage_forward(params, g["g3_x"], layers), g["g3_e_pool"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(co.pinsage_forward(params, g["g3_x"], None), g["g3_e_mlp"], rtol=1e-5, atol=1e-6)


def test_lsh_encode_matches_numpy_fma_emulation():
    rs = np.random.RandomState(2)
    x = rs.standard_normal((300, 48)).astype(np.float32)
    A = orc.lsh_rotation_matrix(48, 128)
    codes, _ = orc.lsh_encode(x, A)
    assert np.array_equal(co.lsh_encode(x, A, threads=2), codes)


def test_hamming_and_dot_topk():
    rs = np.random.RandomState(3)
    codes = rs.randint(0, 256, size=(500, 8)).astype(np.uint8)
    codes[100] = codes[7]; codes[300] = codes[7]              # exact ties -> id order
    d0, i0 = orc.hamming_topk(codes[:20], codes, 11)
    d1, i1 = co.hamming_topk(codes[:20], codes, 11, threads=2)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    assert i1[7, :3].tolist() == [7, 100, 300]
    E = rs.standard_normal((400, 24)).astype(np.float32)
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    q = np.array([0, 5, 399])
    v, i = co.dot_topk(E, q, 11)
    for r, qi in enumerate(q):
        _, ref = orc.exact_topk(E, int(qi), 11)
        assert np.array_equal(i[r], ref)


@pytest.mark.parametrize("cs,N,nq,k,kind", [
    (128, 1000, 7, 64, "random"), (128, 700, 5, 64, "few"), (128, 300, 5, 64, "same"),      # 1024-bit codes, a full wave of k
    (128, 40, 5, 64, "random"), (32, 5, 3, 40, "few"), (4, 1, 4, 5, "same"), (4, 63, 5, 64, "random"),   # N < k: padding
    (128, 0, 3, 64, "random"), (4, 0, 1, 1, "same"),                                        # empty table: padding only
    (4, 3000, 9, 33, "few"), (64, 257, 5, 17, "same"), (16, 700, 9, 63, "few"),
])
def test_hamming_references_agree(cs, N, nq, k, kind):
    """The two references that tests/test_hip_hamming_popcount.py holds the popcount kernel to -- this C oracle and the numpy
    restatement written there (unpackbits of the XOR, lexsort by (distance, id)) -- agree bit for bit where the GPU tests
    rely on them alone: 1024-bit codes with k = 64, N < k and N = 0 (the oracle accepts an empty table and pads every
    position itself), one repeated code and a handful of distinct codes, with and without an id offset."""
    from test_hip_hamming_popcount import INT_MAX, cut_and_offset, make_case, np_hamming_topk, oracle_hamming_topk, plant_positions
    q, codes, pos = make_case(cs, N, nq, kind, seed=cs + N + k)
    assert pos == plant_positions(N) and codes.shape == (N, cs) and q.shape == (nq, cs)
    ref = np_hamming_topk(q, codes, 64)
    kk = min(k, N)
    for off in (0, 2 ** 33 + 5):
        dn, idn = cut_and_offset(ref, k, off)
        do, ido = oracle_hamming_topk(q, codes, k, off)
        assert dn.dtype == do.dtype == np.int32 and idn.dtype == ido.dtype == np.int64
        assert np.array_equal(dn, do) and np.array_equal(idn, ido)
        assert np.all(do[:, kk:] == INT_MAX) and np.all(ido[:, kk:] == -1)
        assert np.all(ido[:, :kk] >= off) and np.all(ido < N + off)
        # the oracle's own padding and offset, untouched by the wrapper
        rd, ri = co.hamming_topk(q, codes, k, id_offset=off, threads=3)
        assert np.array_equal(ri, ido) and np.all(rd[:, kk:] == np.float32(2147483647.0))
        assert np.array_equal(rd[:, :kk].astype(np.int32), do[:, :kk])
    lead = (list(range(N)) if kind == "same" else pos)[:k]
    assert ref[1][0, :len(lead)].tolist() == lead and not ref[0][0, :len(lead)].any()


def test_ranking_losses_by_hand():
    """B = 3, N = 2, D = 2, margin 1/2, grad_out 3/2 (g = 1/2): every number is exact and small enough to check on paper.  Signs of
    zeros are part of the contract: an inactive row's -g p is -0.0 and t + (-0.0) is +0.0."""
    f = np.float32
    bits = lambda a: np.ascontiguousarray(a, dtype=f).view(np.int32).tolist()      # noqa: E731
    Q = np.array([[1, 2], [0.5, -1], [2, 0]], dtype=f)
    P = np.array([[1, 1], [2, 0.5], [-1, 3]], dtype=f)
    X = np.array([[1, 0], [0, 1]], dtype=f)
    # shared candidates: similarities [[1, 2], [.5, -1], [2, 0]]; positives 3, .5, -2; l = -.5 (inactive), .5, 4.5
    sim, idx = co.hardest_negative(Q, X)
    assert sim.tolist() == [2.0, 0.5, 2.0] and idx.tolist() == [1, 0, 0]
    row_loss, active, loss = co.margin_loss(Q, P, sim, 0.5)
    assert row_loss.tolist() == [0.0, 0.5, 4.5] and active.tolist() == [0, 1, 1] and loss == f(5.0) / f(3.0)
    g = co.margin_loss_bwd(Q, P, X, 0, idx, active, 1.5)
    assert bits(g["dQ"]) == bits([[0.0, 0.0], [-0.5, -0.25], [1.0, -1.5]])         # row 1: .5 (1, 0) - .5 (2, .5)
    assert bits(g["dP"]) == bits([[-0.0, -0.0], [-0.25, 0.5], [-1.0, -0.0]])
    assert bits(g["dX"]) == bits([[1.25, -0.5], [0.0, 0.0]])                       # .5 Q_1 + .5 Q_2; row 0 is inactive
    assert set(co.margin_loss_bwd(Q, P, X, 0, idx, active, 1.5, want=("dX",))) == {"dX"}
    # per-query candidates, every row with the same two: the same pairs, dX [3, 2, 2] with the hit filled in
    X3 = np.ascontiguousarray(np.broadcast_to(X, (3, 2, 2)))
    sim3, idx3 = co.hardest_negative(Q, X3, per_query=True)
    assert bits(sim3) == bits(sim) and idx3.tolist() == idx.tolist()
    g3 = co.margin_loss_bwd(Q, P, X3, 1, idx, active, 1.5)
    assert bits(g3["dQ"]) == bits(g["dQ"]) and bits(g3["dP"]) == bits(g["dP"])
    assert bits(g3["dX"]) == bits([[[0, 0], [0, 0]], [[0.25, -0.5], [0, 0]], [[1.0, 0.0], [0, 0]]])
    # batch-hard: Q P^T = [[3, 3, 5], [-.5, .5, -3.5], [2, 4, -2]] without its diagonal; l = 2.5, -.5 (inactive), 6.5
    simh, idxh = co.hardest_negative(Q, P, exclude_diag=True)
    assert simh.tolist() == [5.0, -0.5, 4.0] and idxh.tolist() == [2, 0, 1]
    row_loss, active, loss = co.margin_loss(Q, P, simh, 0.5)
    assert row_loss.tolist() == [2.5, 0.0, 6.5] and active.tolist() == [1, 0, 1] and loss == f(3.0)
    gh = co.margin_loss_bwd(Q, P, None, 2, idxh, active, 1.5)
    assert set(gh) == {"dQ", "dP"}
    assert bits(gh["dQ"]) == bits([[-1.0, 1.0], [0.0, 0.0], [1.5, -1.25]])         # .5 P_2 - .5 P_0;  0;  .5 P_1 - .5 P_2
    assert bits(gh["dP"]) == bits([[-0.5, -1.0], [1.0, 0.0], [-0.5, 1.0]])         # -g_j Q_j + .5 Q_b over active b with a_b = j
    # a row without a candidate
    s1, i1 = co.hardest_negative(Q[:1], P[:1], exclude_diag=True)
    assert s1[0] == -np.inf and i1[0] == -1
