"""utils.evaluation drop-in and the rank kernels behind it (ps_row_dot, ps_rank_count = the GEMM with the counting epilogue).

  * ranks bit-exact against torch on a dense.linear slab under (key, id) order (run.py's shape, D = 256, unaligned D, one
    query, a tie-heavy catalogue), thr bit-equal to the slab entry, rank <= k exactly when dot_topk returns the item,
    item-range counts (id_offset) adding up to the whole-catalogue count;
  * the drop-in against the reference's own outputs (tests/golden/reference_golden_eval.npz, tests/golden/make_golden_eval.py):
    equal floats, MRR bit for bit, the reference's dict keys, return types and signatures; its edge semantics;
  * CPU only: the module imports (the reference's run.py / main.py stop at `import utils.evaluation` without it) and the C
    entries reject invalid arguments before touching a device.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_golden_eval.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------------- CPU only

def test_evaluation_module_imports():
    import utils.evaluation as ev
    import utils.nearest_neighbors as nn
    for name in ("calculate_hit_rate", "calculate_mrr", "evaluate_embeddings", "generate_recommendations"):
        assert callable(getattr(ev, name))
    assert ev.generate_recommendations is nn.generate_recommendations


def test_signatures_match_reference(gold):
    import inspect
    import utils.evaluation as ev
    for name in ("calculate_hit_rate", "calculate_mrr", "evaluate_embeddings", "generate_recommendations"):
        assert str(inspect.signature(getattr(ev, name))) == str(gold[f"e3_sig_{name}"]), name


def test_rank_entries_reject_invalid_arguments():
    from pinsage_hip import native
    if not native.have_lib():
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(native.SO_PATH)
    i64, i32, p = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    one = p(16)       # never dereferenced: every call below returns before any device work
    rc = lambda *a: lib.ps_rank_count(*a)                                                    # noqa: E731
    assert rc(one, i64(-1), i32(8), i64(0), one, i64(4), one, one, one, p(0)) == native.PS_EINVAL
    assert rc(one, i64(10), i32(0), i64(0), one, i64(4), one, one, one, p(0)) == native.PS_EINVAL
    assert rc(one, i64(10), i32(8), i64(0), one, i64(-4), one, one, one, p(0)) == native.PS_EINVAL
    assert rc(p(0), i64(10), i32(8), i64(0), one, i64(4), one, one, one, p(0)) == native.PS_EINVAL
    assert rc(one, i64(10), i32(8), i64(0), one, i64(4), one, one, p(0), p(0)) == native.PS_EINVAL
    assert rc(one, i64(10), i32(8), i64(0), one, i64(4), one, one, p(20), p(0)) == native.PS_EINVAL   # count not 8-B aligned
    assert rc(one, i64(1 << 31), i32(8), i64(0), one, i64(4), one, one, one, p(0)) == native.PS_EUNSUPPORTED
    assert rc(p(0), i64(0), i32(8), i64(0), p(0), i64(4), p(0), p(0), p(0), p(0)) == native.PS_OK   # nothing to count
    rd = lambda *a: lib.ps_row_dot(*a)                                                       # noqa: E731
    assert rd(one, i64(10), one, i64(10), i32(0), one, one, i64(3), one, p(0)) == native.PS_EINVAL
    assert rd(one, i64(10), one, i64(10), i32(8), one, one, i64(-1), one, p(0)) == native.PS_EINVAL
    assert rd(one, i64(10), p(0), i64(10), i32(8), one, one, i64(3), one, p(0)) == native.PS_EINVAL
    assert rd(p(0), i64(10), p(0), i64(10), i32(8), p(0), p(0), i64(0), p(0), p(0)) == native.PS_OK


# ---------------------------------------------------------------------------------------------------------- GPU

def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _order_key(v):
    """the kernels' order key: int32, increasing in the float's total order (larger key = earlier in ps_dot_topk's order)"""
    b = v.contiguous().view(torch.int32)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def _slab_ranks(E, q, gt, chunk=1024):
    """(rank, thr, pairs whose target ties with another item) from a dense.linear(E[q], E) slab: 1 + #{j : key_j > key_gt or (key_j == key_gt and j < gt)}"""
    from pinsage_hip import dense
    N = E.size(0)
    cols = torch.arange(N, device=E.device)
    ranks, thrs, tied = [], [], 0
    for s in range(0, q.numel(), chunk):
        qq, gg = q[s:s + chunk], gt[s:s + chunk]
        S = dense.linear(E.index_select(0, qq).contiguous(), E)
        thr = S.gather(1, gg[:, None])
        K = _order_key(S)
        kt = K.gather(1, gg[:, None])
        c = (K > kt).sum(1) + ((K == kt) & (cols[None, :] < gg[:, None])).sum(1)
        tied += int(((K == kt).sum(1) > 1).sum())
        ranks.append(c + 1)
        thrs.append(thr[:, 0])
        del S, K
    return torch.cat(ranks), torch.cat(thrs), tied


def _unit_rows(N, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn(N, D, generator=g)
    return torch.nn.functional.normalize(X, dim=1).to(_dev()).contiguous()


def _tie_heavy(N, D, seed):
    """values on five levels, duplicated rows, all-zero rows, a -0.0 row: many exact ties"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = (torch.randint(-2, 3, (N, D), generator=g).float() * 0.5)
    X[100:200] = X[0:100]
    X[300:340] = 0.0
    X[341] = -0.0
    X[N - 50:] = X[10:60]
    return X.to(_dev()).contiguous()


def _pairs(N, nq, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randint(0, N, (nq,), generator=g)
    gt = torch.randint(0, N, (nq,), generator=g)
    gt[: nq // 10] = q[: nq // 10]                               # ground truth = the query itself
    return q.to(_dev()), gt.to(_dev())


CASES = [
    # name, N, D, nq, data
    ("run_py_shape", 59047, 128, 5000, "unit"),
    ("d256", 59047, 256, 2000, "unit"),
    ("unaligned_d100", 1000 + 37, 100, 1, "unit"),
    ("unaligned_d100_many", 4099, 100, 333, "unit"),
    ("small_n", 77, 32, 50, "unit"),
    ("ties", 4099, 64, 700, "ties"),
    ("ties_unaligned", 2053, 36, 300, "ties"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,N,D,nq,data", CASES, ids=[c[0] for c in CASES])
def test_target_rank_bit_exact_vs_slab(name, N, D, nq, data):
    from pinsage_hip import dense
    E = _unit_rows(N, D, 11) if data == "unit" else _tie_heavy(N, D, 12)
    q, gt = _pairs(N, nq, 13)
    want_rank, want_thr, tied = _slab_ranks(E, q, gt)
    thr = dense.row_dot(E, q, E, gt)
    assert torch.equal(thr.view(torch.int32), want_thr.contiguous().view(torch.int32)), "ps_row_dot != slab entry"
    rank = dense.target_rank(E, q, gt)
    assert rank.dtype == torch.int64 and rank.is_cuda
    assert torch.equal(rank, want_rank)
    if data == "ties":
        assert tied > nq // 4, "the tie-heavy case should exercise the id order"


@pytest.mark.gpu
@pytest.mark.parametrize("data", ["unit", "ties"])
def test_rank_consistent_with_dot_topk(data):
    from pinsage_hip import dense
    N, D, nq = (59047, 128, 1000) if data == "unit" else (4099, 64, 500)
    E = _unit_rows(N, D, 21) if data == "unit" else _tie_heavy(N, D, 22)
    q, gt = _pairs(N, nq, 23)
    if data == "unit":                                            # some ground truths among the query's nearest items
        _, near = dense.dot_topk(E, q[:200], 40, exclude_self=False)
        gt[:200] = near[torch.arange(200, device=E.device), torch.arange(200, device=E.device) % 40]
    rank = dense.target_rank(E, q, gt)
    _, ids = dense.dot_topk(E, q, 500, exclude_self=False)
    for k in (1, 10, 50, 100, 500):
        hit = (ids[:, :k] == gt[:, None]).any(1)
        assert torch.equal(rank <= k, hit), k
    assert int((rank <= 10).sum()) > 0 and int((rank > 500).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("data", ["unit", "ties"])
def test_item_range_counts_add_up(data):
    from pinsage_hip import dense
    N, D, nq = (9001, 128, 777) if data == "unit" else (4099, 64, 600)
    E = _unit_rows(N, D, 31) if data == "unit" else _tie_heavy(N, D, 32)
    q, gt = _pairs(N, nq, 33)
    Q = E.index_select(0, q).contiguous()
    thr = dense.row_dot(E, q, E, gt)
    whole = dense.rank_count(E, Q, thr, gt)
    count = torch.zeros(nq, dtype=torch.int64, device=E.device)
    for a, b in ((0, 1234), (1234, 3001), (3001, N)):
        dense.rank_count(E[a:b], Q, thr, gt, id_offset=a, count=count)
    assert torch.equal(count, whole)
    assert torch.equal(whole + 1, dense.target_rank(E, q, gt))


def _gold_E(gold, device=None):
    E = torch.from_numpy(gold["e1_E16"].astype(np.float32))
    return E if device is None else E.to(device)


@pytest.mark.gpu
def test_dropin_matches_reference(gold):
    import utils.evaluation as ev
    E = _gold_E(gold)                                             # CPU fp32, as run.py passes it
    pairs = gold["e1_pairs"]
    q, gt = pairs[:, 0], pairs[:, 1]
    from pinsage_hip import dense
    rank = dense.target_rank(E.to(_dev()), torch.from_numpy(q), torch.from_numpy(gt))
    assert np.array_equal(rank.cpu().numpy(), gold["e1_ranks_f64"])
    for k in (1, 5, 10, 50, 100, 500, 2000):
        h = ev.calculate_hit_rate(E, q, gt, k=k)
        assert type(h) is float and h == float(gold[f"e1_hit_{k}"]), k
    assert ev.calculate_hit_rate(E, q, gt) == float(gold["e1_hit_default"])
    for s in (1, 7.5, 100):
        m = ev.calculate_mrr(E, q, gt, scale=s)
        assert type(m) is np.float64 and m.tobytes() == gold[f"e1_mrr_{s}"].tobytes(), s
    assert ev.calculate_mrr(E, q, gt).tobytes() == gold["e1_mrr_default"].tobytes()
    test_data = {"positive_pairs": torch.from_numpy(pairs)}
    for tag, res in (("default", ev.evaluate_embeddings(E, test_data)),
                     ("custom", ev.evaluate_embeddings(E, test_data, k_values=[1, 3, 1000]))):
        assert list(res.keys()) == list(gold[f"e1_eval_{tag}_keys"])
        assert [type(v).__name__ for v in res.values()] == list(gold[f"e1_eval_{tag}_types"])
        assert np.array([np.float64(v) for v in res.values()]).tobytes() == gold[f"e1_eval_{tag}_values"].tobytes()
    # list inputs, device embeddings
    assert ev.calculate_hit_rate(E.to(_dev()), list(q), list(gt), k=50) == float(gold["e1_hit_50"])


@pytest.mark.gpu
def test_generate_recommendations_matches_reference(gold):
    import utils.evaluation as ev
    E = _gold_E(gold)
    rq = gold["e2_rec_queries"]
    for (k, excl), a in zip(((10, True), (25, False), (1, True)), rq):
        got = ev.generate_recommendations(E, int(a), k=k, exclude_query=excl)
        assert np.array_equal(np.asarray(got), gold[f"e2_rec_{k}_{int(excl)}"]), (k, excl)
    assert np.array_equal(np.asarray(ev.generate_recommendations(E, int(rq[0]))), gold["e2_rec_default"])


@pytest.mark.gpu
def test_one_rank_launch_per_evaluation(gold):
    import utils.evaluation as ev
    from pinsage_hip import native as nv
    E = _gold_E(gold, _dev())
    test_data = {"positive_pairs": torch.from_numpy(gold["e1_pairs"])}
    timer = nv.KernelTimer()
    nv.set_timer(timer)
    try:
        ev.evaluate_embeddings(E, test_data)
    finally:
        nv.set_timer(None)
    calls = timer.summary()
    assert calls["ps_rank_count"]["launches"] == 1 and calls["ps_row_dot"]["launches"] == 1
    assert "ps_dot_topk" not in calls and "ps_linear" not in calls


@pytest.mark.gpu
def test_edge_semantics(gold):
    import utils.evaluation as ev
    E = _gold_E(gold)
    N = E.size(0)
    pairs = gold["e1_pairs"][:40]
    q, gt = pairs[:, 0], pairs[:, 1]
    with pytest.raises(RuntimeError):
        ev.calculate_hit_rate(E, q, gt, k=N + 1)
    with pytest.raises(RuntimeError):
        ev.evaluate_embeddings(E, {"positive_pairs": torch.from_numpy(pairs)}, k_values=[10, N + 1])
    assert ev.calculate_hit_rate(E, q, gt, k=N) == 1.0
    assert ev.calculate_hit_rate(E, q, gt, k=0) == 0.0
    with pytest.raises(ZeroDivisionError):
        ev.calculate_hit_rate(E, [], [], k=10)
    with pytest.raises(ZeroDivisionError):
        ev.evaluate_embeddings(E, {"positive_pairs": torch.zeros((0, 2), dtype=torch.int64)})
    # negative query indices wrap, as item_embeddings[query_idx] does
    assert ev.calculate_hit_rate(E, q - N, gt, k=50) == ev.calculate_hit_rate(E, q, gt, k=50)
    assert ev.calculate_mrr(E, q - N, gt).tobytes() == ev.calculate_mrr(E, q, gt).tobytes()
    with pytest.raises(IndexError):
        ev.calculate_hit_rate(E, np.array([N]), np.array([0]), k=10)
    # a ground truth that is no item index: never in the top k (a miss); the reference's MRR finds no position (IndexError)
    bad = gt.copy()
    bad[0] = -1
    assert ev.calculate_hit_rate(E, q, bad, k=N) == 39 / 40
    with pytest.raises(IndexError):
        ev.calculate_mrr(E, q, bad)
