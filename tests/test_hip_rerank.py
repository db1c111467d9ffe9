"""ps_rerank_topk (csrc/rerank.hip) on the device against tests/helpers/rerank_cases.py's restatement, bit for bit, over its case
table; against the exact search (dense.dot_topk) when the candidates are all other items, also with NaN, +inf and -0.0 rows in
the table; its error paths; and the two-level search of utils.nearest_neighbors.LSHIndex (refine_factor) on the recall fixture:
equal to the restatement over the candidates an unrefined twin index returns, never fewer hits than the Hamming order for any
query and more on average."""
import numpy as np
import pytest
import torch

from helpers import abi_cases as ac
from helpers import abi_cases_rerank  # noqa: F401  (the entry point joins ac.CASES)
from helpers import rerank_cases as rc

pytestmark = pytest.mark.gpu
CANARY = 7.0


def _dev(a, offset=0):
    """a on the device; offset: that many floats into a larger, 16-byte aligned buffer"""
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.tensor(a).cuda()
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.tensor(a))
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t


def _np(pair):
    return tuple(t.cpu().numpy() for t in pair)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_case_is_the_restatement(name):
    from pinsage_hip import dense
    c = rc.cases()[name]
    cand = torch.tensor(c.cand).cuda()
    got = _np(dense.rerank_topk(_dev(c.E, c.offset), _dev(c.Q, c.offset), cand, c.k, id_offset=c.id_offset))
    assert rc.same(got, rc.expected(name))
    if c.offset:                                                    # unaligned views: the bits of the aligned copy
        E, Q = _dev(c.E), _dev(c.Q)
        assert E.data_ptr() % 16 == 0 and Q.data_ptr() % 16 == 0
        assert rc.same(_np(dense.rerank_topk(E, Q, cand, c.k, id_offset=c.id_offset)), got)


def _all_others(n, seed):
    """int64 [n, n - 1]: row i = a random permutation of every id but i"""
    rs = np.random.RandomState(seed)
    return np.stack([np.delete(np.arange(n), i)[rs.permutation(n - 1)] for i in range(n)]).astype(np.int64)


@pytest.mark.parametrize("special", [False, True])
def test_all_other_items_as_candidates_is_the_exact_search(special):
    """E [300, 32], the queries are its rows, every row's candidates are all OTHER ids in random order, k = 17: the result is
    dense.dot_topk(E, qidx, 17, exclude_self=True), values and ids.

    One slot needs care.  exclude_self does not drop the query's own item, it ranks it as (-inf, self), and that entry precedes
    every similarity whose key lies below -inf: a NaN with the sign bit set.  With the +inf row as the query every other
    similarity is inf - inf = 0xffc00000 on this hardware, so the exact search lists (-inf, 41) in slot 1 of row 41 (measured: the
    16 slots behind it are the re-rank's, shifted by one), and a candidate list that does not hold the query's id cannot.  The
    expectation is therefore the exact search's first 18 with the query's own entry taken out where it occurs, cut to 17: the
    exact search's order over the other items.  Without special values the own entry never occurs and this is plain equality."""
    from pinsage_hip import dense
    n, k = 300, 17
    E = np.random.RandomState(51).standard_normal((n, 32)).astype(np.float32)
    if special:                                                     # the order on special values, without restating it
        E[40], E[41], E[42] = np.nan, np.inf, -0.0
    E = _dev(E)
    qidx = torch.arange(n, device="cuda")
    cand = torch.tensor(_all_others(n, 52)).cuda()
    v18, i18 = _np(dense.dot_topk(E, qidx, k + 1, exclude_self=True))
    own = i18 == np.arange(n)[:, None]
    assert sorted(np.flatnonzero(own.any(axis=1)).tolist()) == ([41] if special else [])
    assert np.isneginf(v18[own]).all()
    keep = np.stack([np.flatnonzero(~row)[:k] for row in own])
    want = np.take_along_axis(v18, keep, axis=1), np.take_along_axis(i18, keep, axis=1)
    if not special:
        assert rc.same(want, _np(dense.dot_topk(E, qidx, k, exclude_self=True)))
    got = _np(dense.rerank_topk(E, E, cand, k))
    if special:
        bits = want[0].view(np.uint32)                              # NaN of either sign: first and last in the order
        assert (bits[:, 0] == 0x7fc00000).all() and (bits[41, 1:] == 0xffc00000).all() and np.isinf(v18).any()
    assert rc.same(got, want)


def test_error_paths():
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    lim = nv.lib().ps_rerank_max_candidates()
    assert lim == dense.rerank_max_candidates() >= rc.MIN_LIMIT
    N, D, nq = 20, 8, 3
    E, Q = _dev(np.ones((N, D), np.float32)), _dev(np.ones((nq, D), np.float32))
    cand = torch.zeros((nq, lim + 1), dtype=torch.int64, device="cuda")
    vals = torch.full((nq, 4), CANARY, dtype=torch.float32, device="cuda")
    ids = torch.full((nq, 4), 77, dtype=torch.int64, device="cuda")

    def call(R, k, e=E, n=N, d=D):
        rc_ = nv.lib().ps_rerank_topk(nv.ptr(e), n, d, 0, nv.ptr(Q), nq, nv.ptr(cand), R, k, nv.ptr(vals), nv.ptr(ids), nv.stream())
        torch.cuda.synchronize()
        return rc_
    assert call(0, 4) == nv.PS_EUNSUPPORTED and call(lim + 1, 4) == nv.PS_EUNSUPPORTED and call(-1, 4) == nv.PS_EUNSUPPORTED
    assert call(5, 4, n=2 ** 31) == nv.PS_EUNSUPPORTED
    assert call(5, 0) == nv.PS_EINVAL and call(5, -1) == nv.PS_EINVAL and call(5, 4, d=0) == nv.PS_EINVAL
    assert call(5, 4, n=-1) == nv.PS_EINVAL and call(5, 4, e=None) == nv.PS_EINVAL
    assert (vals == CANARY).all() and (ids == 77).all()             # a refused call writes nothing
    assert call(5, 4) == nv.PS_OK and (ids[:, 0] == 0).all() and (ids[:, 1:] == -1).all() and (vals[:, 0] == D).all()
    # the wrapper: CPU tensors raise as row_dot's do; shapes and the limit are named
    cpuE, cpuQ = torch.ones(N, D), torch.ones(nq, D)
    with pytest.raises(nv.NativeError):
        dense.row_dot(cpuE, torch.zeros(1, dtype=torch.int64), cpuE, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(nv.NativeError):
        dense.rerank_topk(cpuE, cpuQ, cand[:, :5].cpu(), 4)
    with pytest.raises(nv.NativeError):
        dense.rerank_topk(E, cpuQ, cand[:, :5], 4)
    with pytest.raises(TypeError):
        dense.rerank_topk(E.double(), Q, cand[:, :5], 4)
    with pytest.raises(ValueError, match=str(lim)):
        dense.rerank_topk(E, Q, cand, 4)
    with pytest.raises(ValueError):
        dense.rerank_topk(E, Q, cand[:2, :5], 4)
    with pytest.raises(ValueError):
        dense.rerank_topk(E, Q, cand[:, :5], 0)


def test_contract_matrix_holds_the_rerank():
    """The contract matrix of tests/test_hip_abi_contract.py (captured stream, poisoned outputs, guard bands, replays) for the entry
    point, started from here as well: that module parametrises over the case table when it is collected, and a run of it alone
    does not import the case module of this entry point."""
    import test_hip_abi_contract as contract
    assert "ps_rerank_topk" in ac.CASES
    contract.test_contract("ps_rerank_topk")


# ---- the two-level search of LSHIndex --------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def indexes():
    """(refined index with factor 1 -- each test sets its own --, its unrefined twin: same rotation, same items)"""
    from utils.nearest_neighbors import LSHIndex
    x, _ = rc.recall_fixture()
    twin = LSHIndex(64, rc.RECALL_BITS)
    twin.build(np.array(x))
    refined = LSHIndex(64, rc.RECALL_BITS)
    refined.refine_factor = 1
    refined.build(np.array(x))
    assert torch.equal(refined.index.A, twin.index.A) and torch.equal(refined.index.codes, twin.index.codes)
    return refined, twin


def test_default_keeps_no_vectors(indexes):
    from utils.nearest_neighbors import LSHIndex
    refined, twin = indexes
    assert LSHIndex.refine_factor == 0 and twin.refine_factor == 0 and twin.index.xb is None
    x, _ = rc.recall_fixture()
    assert refined.index.xb is not None and np.array_equal(refined.index.xb.cpu().numpy(), x)


@pytest.mark.parametrize("k,factor,scan", [(5, 4, "ps_hamming_topk_mfma_codes"), (5, 10, "ps_hamming_topk"), (10, 10, "ps_l2_topk")])
def test_two_level_search_on_the_fixture(indexes, monkeypatch, k, factor, scan):
    from pinsage_hip import dense
    refined, twin = indexes
    x, q = rc.recall_fixture()
    assert (k, factor) in rc.RECALL_SETTINGS
    R = factor * k
    monkeypatch.setattr(refined, "refine_factor", factor)
    spy = _Spy(monkeypatch)
    vals, ids = refined.search(np.array(q), k)
    names = spy.take()
    assert scan in names and names[-1] == "ps_rerank_topk"         # R = 20: MFMA scan, 50: popcount scan, 100: the large-k form
    dv, di = refined.search_device(torch.tensor(np.array(q)).cuda(), k)
    assert vals.dtype == np.float32 and ids.dtype == np.int64 and dv.is_cuda and di.is_cuda
    assert rc.same((vals, ids), _np((dv, di)))
    # equal to the restatement over the candidates of the unrefined twin at k = R
    _, cand = twin.search(np.array(q), R)
    _, first = twin.search(np.array(q), k)
    assert cand.shape == (64, R) and np.array_equal(first, cand[:, :k])
    assert rc.same((vals, ids), rc.restate(x, q, cand, k, sims=rc.recall_sims()))
    assert (np.diff(vals, axis=1) <= 0).all()
    # hits against the exact search's truth
    truth = dense.dot_topk(torch.tensor(np.array(x)).cuda(), torch.arange(64), k, exclude_self=False)[1].cpu().numpy()
    assert np.array_equal(truth, rc.recall_truth(k))
    before, after = rc.hits(first, truth), rc.hits(ids, truth)
    print(f"k={k} factor={factor}: recall@k {before.mean() / k:.4f} -> {after.mean() / k:.4f}")
    assert (after >= before).all()
    assert after.mean() > before.mean()


def test_candidates_of_the_whole_index_give_the_exact_search():
    from pinsage_hip import dense
    from utils.nearest_neighbors import LSHIndex
    x = np.array(rc.recall_fixture()[0][100:130])
    ix = LSHIndex(64, rc.RECALL_BITS)
    ix.refine_factor = 10
    ix.build(x)
    vals, ids = ix.search(x, 5)                                     # R = min(50, 30) = ntotal
    want = _np(dense.dot_topk(torch.tensor(x).cuda(), torch.arange(30), 5, exclude_self=False))
    assert rc.same((vals, ids), want)
    vals, ids = ix.search(x[:3], 40)                                # k above ntotal: padded
    assert (ids[:, 30:] == -1).all() and np.isneginf(vals[:, 30:]).all() and (np.sort(ids[:, :30], axis=1) == np.arange(30)).all()


def test_value_errors(indexes):
    from pinsage_hip import dense
    from utils.nearest_neighbors import LSHIndex
    refined, twin = indexes
    _, q = rc.recall_fixture()
    q = np.array(q[:2])
    for bad in (-1, 2.5, 2.0, "3", None, True):
        ix = LSHIndex(64, rc.RECALL_BITS)
        ix.refine_factor = bad
        with pytest.raises(ValueError, match="refine_factor"):
            ix.build(q)
        assert ix.index.ntotal == 0
    late = LSHIndex(64, rc.RECALL_BITS)
    late.build(q)
    late.refine_factor = 3                                          # after a build that kept no vectors
    with pytest.raises(ValueError, match="before build"):
        late.search(q, 1)
    with pytest.raises(ValueError, match="before build"):
        late.search_device(torch.tensor(q).cuda(), 1)
    late.refine_factor = 0
    assert late.search(q, 1)[1].tolist() == [[0], [1]]
    lim = dense.rerank_max_candidates()
    assert lim < refined.index.ntotal
    big = LSHIndex(64, rc.RECALL_BITS)
    big.index = refined.index                                       # the fixture's table and vectors
    big.refine_factor = lim // 100 + 1
    with pytest.raises(ValueError, match=str(lim)):
        big.search(q, 100)


def test_benchmark_reports_the_refined_method():
    from utils.nearest_neighbors import benchmark_search_methods
    x, q = rc.recall_fixture()
    res = benchmark_search_methods(np.array(x), np.array(q), k=10, methods=["exact", "lsh", "lsh_refine"])
    assert list(res) == ["exact", "lsh", "lsh_refine"] and res["lsh_refine"]["method"] == "LSH + exact re-rank"
    assert res["lsh_refine"]["index_size"] == len(x) and res["lsh_refine"]["indices"].shape == (64, 10)
    print(f"recall@10: lsh {res['lsh']['recall']:.4f}, lsh_refine {res['lsh_refine']['recall']:.4f}")
    assert res["lsh_refine"]["recall"] >= res["lsh"]["recall"]
    assert list(benchmark_search_methods(np.array(x[:1000]), np.array(q[:4]), k=3)) == ["exact", "lsh", "ivf"]
