"""tests/helpers/rerank_cases.py on the CPU: every case of the table contains what it is named for, the restatement agrees with a
second, brute-force statement (a Python sort of (key, id) tuples over a set), and on the recall fixture -- codes and Hamming
order from the project's CPU oracle -- re-ranking the Hamming candidates never loses a hit of any query and raises the mean."""
import struct

import numpy as np
import pytest

from helpers import rerank_cases as rc

NAMES = sorted(rc.cases())


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def _geometry(c):
    N, D = c.E.shape
    nq, R = c.cand.shape
    return N, D, nq, R


def _n_valid(c):
    return [len(rc.valid_rows(row, c.E.shape[0], c.id_offset)) for row in c.cand]


# ---- the cases contain what they are named for -----------------------------------------------------------------------------------
def test_the_table_has_the_shapes_the_kernel_branches_on():
    cs = rc.cases()
    assert _geometry(cs["smallest"]) == (5, 1, 1, 1) and cs["smallest"].k == 1
    assert _geometry(cs["d3-scalar-all-emitted"]) == (70, 3, 3, 63) and cs["d3-scalar-all-emitted"].k == 63
    assert _geometry(cs["d4-r64-k1"])[1:] == (4, 3, rc.LANES) and cs["d4-r64-k1"].k == 1
    assert _geometry(cs["d4-r65-k33"])[1:] == (4, 3, rc.LANES + 1) and cs["d4-r65-k33"].k == 33        # a second lane round, k across 32
    assert _geometry(cs["d256-main"]) == (1000, 256, 65, 110) and cs["d256-main"].k == 11
    assert _geometry(cs["limit-R"]) == (5000, 8, 2, rc.limit()) and cs["limit-R"].k == 100
    assert rc.limit() >= rc.MIN_LIMIT
    for name in ("d130-unaligned", "d132-unaligned"):
        c = cs[name]
        assert c.offset == 1 and (c.offset * 4) % 16 != 0          # one float into a 16-byte aligned buffer
    assert cs["d130-unaligned"].E.shape[1] == 130 and 130 % 4 != 0 and 130 > 4 * rc.TILE_COLS and 130 % rc.TILE_COLS not in (0, 1)
    assert cs["d132-unaligned"].E.shape[1] == 132 and 132 % 4 == 0                                     # only the pointers object
    assert all(c.offset == 0 for n, c in cs.items() if "unaligned" not in n)
    # the plain cases hold valid, distinct ids only: what they test is the shape
    for name in ("smallest", "d3-scalar-all-emitted", "d4-r64-k1", "d4-r65-k33", "d130-unaligned", "d132-unaligned", "d256-main",
                 "limit-R"):
        c = cs[name]
        assert _n_valid(c) == [c.cand.shape[1]] * c.cand.shape[0], name
    assert cs["d3-scalar-all-emitted"].k == cs["d3-scalar-all-emitted"].cand.shape[1]                  # everything is emitted


def test_invalid_ids_case():
    c = rc.cases()["invalid-ids"]
    N = c.E.shape[0]
    nv = _n_valid(c)
    assert nv[0] > c.k and 0 < nv[1] < c.k and nv[2] == 1 and nv[3] == 0
    flat = c.cand.reshape(-1)
    assert (flat == -1).any() and (flat >= N).any() and (flat < -1).any() and (flat == N).any()
    assert flat.min() == -2 ** 63 and flat.max() == 2 ** 63 - 1
    pads = np.flatnonzero(c.cand[0] == -1)
    assert len(pads) and pads.max() < c.cand.shape[1] - 1 and (c.cand[0, pads.max() + 1:] >= 0).any()  # a pad INSIDE the list
    v, i = rc.expected(c.name)
    assert (i[3] == -1).all() and np.isneginf(v[3]).all() and (i[1] >= 0).sum() == nv[1] and (i[0] >= 0).all()


def test_duplicates_case():
    c = rc.cases()["duplicates"]
    for row in c.cand:
        ids, counts = np.unique(row, return_counts=True)
        assert (counts == 2).all() and len(ids) < c.k
    assert (c.cand[0, 0::2] == c.cand[0, 1::2]).all() and (c.cand[1, :8] == c.cand[1, 8:]).all()
    v, i = rc.expected(c.name)
    for r in range(len(c.cand)):
        got = i[r][i[r] >= 0]
        assert len(got) == 8 and len(set(got.tolist())) == 8 and (i[r, 8:] == -1).all()


def test_ties_and_signed_zeros_case():
    c = rc.cases()["ties-zeros"]
    sims = rc.similarities(c.E, c.Q)
    b = _bits(sims[0])
    assert set(range(12)) <= set(c.cand[0].tolist())
    assert len({int(x) for x in b[0:4]}) == 1 and len({int(x) for x in b[4:8]}) == 1 and b[0] != b[4]     # equal bits, other ids
    # rows 8 / 9: products +0.0; rows 10 / 11: every product -0.0, so the bare chain ends in -0.0 -- and the exact search's
    # GEMM, which adds an absent bias as +0.0, reports +0.0 for all four
    prod = lambda r: _bits((c.Q[0].astype(np.float64) * c.E[r].astype(np.float64)).astype(np.float32))  # noqa: E731
    assert (prod(8) == 0).all() and (prod(9) == 0).all() and (prod(10) == 0x80000000).all() and (prod(11) == 0x80000000).all()
    assert b[8] == b[9] == b[10] == b[11] == 0x00000000
    v, i = rc.expected(c.name)
    pos = {int(x): p for p, x in enumerate(i[0])}
    assert pos[0] + 3 == pos[1] + 2 == pos[2] + 1 == pos[3] and pos[4] + 3 == pos[5] + 2 == pos[6] + 1 == pos[7]
    assert pos[8] + 1 == pos[9] and pos[9] + 1 == pos[10] and pos[10] + 1 == pos[11]                     # four zeros, by id
    assert all(_bits(v[0])[pos[r]] == 0 for r in (8, 9, 10, 11))


def test_big_offset_case():
    c = rc.cases()["offset-2^33"]
    N = c.E.shape[0]
    assert c.id_offset == 2 ** 33
    assert 3 in c.cand[0] and c.id_offset - 1 in c.cand[0] and c.id_offset + N in c.cand[0]
    v, i = rc.expected(c.name)
    assert (i >= c.id_offset).all() and (i < c.id_offset + N).all()


# ---- the restatement against a brute-force statement ------------------------------------------------------------------------------
def _desc_key(v):
    """position of an fp32 in "largest first": a Python integer from the float's bits, written without topk_cases"""
    (b,) = struct.unpack("<I", np.float32(v).tobytes())
    up = (b ^ 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)          # increasing in the value
    return 0xFFFFFFFF - up


def brute(E, Q, cand, k, id_offset, sims):
    N, nq = E.shape[0], Q.shape[0]
    vals = np.full((nq, k), -np.inf, dtype=np.float32)
    ids = np.full((nq, k), -1, dtype=np.int64)
    for r in range(nq):
        seen = {int(c) for c in cand[r] if 0 <= int(c) - id_offset < N}
        order = sorted((_desc_key(sims[r, i - id_offset]), i) for i in seen)[:k]
        for p, (_, i) in enumerate(order):
            vals[r, p], ids[r, p] = sims[r, i - id_offset], i
    return vals, ids


@pytest.mark.parametrize("name", NAMES)
def test_restate_is_the_brute_force_statement(name):
    c = rc.cases()[name]
    want = brute(c.E, c.Q, c.cand, c.k, c.id_offset, rc.similarities(c.E, c.Q))
    assert rc.same(rc.expected(name), want)


def test_restate_orders_special_values_as_the_brute_force_statement():
    rs = np.random.RandomState(77)
    E = rs.standard_normal((30, 8)).astype(np.float32)
    E[3], E[4], E[5] = np.nan, np.inf, -0.0
    Q = np.ascontiguousarray(E[:6])
    cand = np.stack([rs.permutation(30) for _ in range(6)]).astype(np.int64)
    sims = rc.similarities(E, Q)
    assert np.isnan(sims).any() and np.isinf(sims).any()
    assert rc.same(rc.restate(E, Q, cand, 30, 0, sims=sims), brute(E, Q, cand, 30, 0, sims))


# ---- re-ranking on the recall fixture ---------------------------------------------------------------------------------------------
def test_fixture_is_as_the_tests_describe_it():
    x, q = rc.recall_fixture()
    assert x.shape == (4200, 64) and x.dtype == np.float32 and q.shape == (64, 64) and np.array_equal(q, x[:64])
    assert np.allclose(np.sqrt((x.astype(np.float64) ** 2).sum(1)), 1.0, atol=1e-6)


@pytest.mark.parametrize("k,factor", rc.RECALL_SETTINGS)
def test_reranking_hamming_candidates_raises_recall(k, factor):
    from oracle import c_oracle as co
    from utils.nearest_neighbors import lsh_rotation_matrix
    x, q = rc.recall_fixture()
    A = lsh_rotation_matrix(64, rc.RECALL_BITS)
    codes = co.lsh_encode(x, A)
    R = min(factor * k, len(x))
    _, cand = co.hamming_topk(codes[:64], codes, R)
    _, first = co.hamming_topk(codes[:64], codes, k)
    assert np.array_equal(first, cand[:, :k])
    truth = rc.recall_truth(k)
    _, second = rc.restate(x, q, cand, k, sims=rc.recall_sims())
    before, after = rc.hits(first, truth), rc.hits(second, truth)
    print(f"k={k} factor={factor}: recall@k {before.mean() / k:.4f} -> {after.mean() / k:.4f}")
    assert (after >= before).all()
    assert after.mean() > before.mean()
