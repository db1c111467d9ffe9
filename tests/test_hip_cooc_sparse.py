"""The sparse producer of the item co-occurrence records (csrc/cooc_sparse.hip: ps_cooc_pairs_sparse) and the `method` switch of
pinsage_hip.cooc.item_cooccurrence_graph / data.graph_builder.GraphBuilder.cooc_method.

Oracles: tests/helpers/cooc_defs.py (the reference restated) and tests/golden/reference_golden_cooc.npz (the reference's own
outputs).  Every comparison is np.array_equal on edge_index (int64) and edge_weight (float32): both producers are exact.

  * CPU: every generated case has the property it is named for (cooc_sparse_cases + cooc_defs.pair_table); the entry rejects
    bad arguments before any device work; an unknown method raises;
  * GPU: golden frames through GraphBuilder(cooc_method="sparse"); sparse == restatement == dense at shapes with planted
    first users at the window boundaries; accumulator overflow at forced capacities 1 / 3 / 8 / default; inputs beyond the
    dense limits (multiplicity 4099 and 128, an odd count above 2^24); `auto` routing; the capacity rerun; trivial inputs and
    thresholds nothing passes; the sparse graph feeds RandomWalkSampler like the dense one.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_golden_cooc.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import cooc_sparse_cases as cases  # noqa: E402

THRESHOLDS = (1, 3, 5, 2.5, 10 ** 6)
WIDE = ("shape", 1100, 6000, 9000, 2)            # more items than the default accumulator has slots: rows start hashed


# ---------------------------------------------------------------------------------------------------------- CPU only

@pytest.mark.parametrize("U,M,R,maxm,thr", cases.SHAPES + [WIDE[1:] + (1,)])
def test_shape_cases_hold_the_planted_first_users(U, M, R, maxm, thr):
    users, items, _ = cases.rows(("shape", U, M, R, maxm))
    assert np.unique(users).size == U and not np.array_equal(users, np.sort(users))
    assert U % cases.WINDOW != 0 and (U - 1) // cases.WINDOW >= 2 and U - 1 > 1030
    t = cases.table(("shape", U, M, R, maxm))
    firsts = {(int(a), int(b)): int(u) for a, b, u in zip(t["a"], t["b"], t["u"])}
    for pair, (u, _) in cases.planted_pairs(U, M).items():
        assert firsts[pair] == u, (pair, firsts[pair], u)
    mult = np.unique(users * M + items, return_counts=True)[1]
    assert mult.max() == maxm
    assert (t["a"] == t["b"]).any() == (maxm > 1)
    ei, _ = cases.restated(("shape", U, M, R, maxm), thr)
    assert 0 < ei.shape[1] // 2 <= t["a"].size               # the threshold keeps some pairs (and drops some when > 1)
    if thr > 1:
        assert ei.shape[1] // 2 < t["a"].size


def test_overflow_case_row_0_has_39_partners():
    users, items, M = cases.overflow()
    t = cases.table(("overflow",))
    partners = np.unique(t["b"][(t["a"] == 0) & (t["b"] > 0)])
    assert M == 40 and partners.size == 39
    assert all(partners.size > s for s in cases.OVERFLOW_SLOTS if s)
    assert (t["a"] == t["b"]).any()                          # self pairs ride along
    per_row = np.bincount(t["a"][t["a"] < t["b"]], minlength=M)
    assert (per_row[:30] > 8).all()                          # every early row overflows every forced capacity


def test_beyond_dense_case_counts():
    users, items, M = cases.beyond_dense()
    t = cases.table(("beyond",))
    count = {(int(a), int(b)): int(c) for a, b, c in zip(t["a"], t["b"], t["count"])}
    assert count[(2, 5)] == 4099 * 4099 + 1 == 16801802 and count[(2, 5)] > 2 ** 24
    assert count[(2, 7)] == 4099 * 4097 and count[(2, 7)] % 2 == 1 and count[(2, 7)] > 2 ** 24
    assert float(np.float32(count[(2, 7)])) != count[(2, 7)]             # edge_weight has to round it
    assert count[(2, 2)] == 4099 * 4098 // 2
    mult = np.unique(users * M + items, return_counts=True)[1]
    assert mult.max() == 4099 > 127
    u128, i128, M128 = cases.multiplicity_128()
    assert np.unique(u128 * M128 + i128, return_counts=True)[1].max() == 128


def test_rerun_case_has_more_pairs_than_the_forced_capacities():
    assert cases.restated(("rerun",), 1)[0].shape[1] // 2 > 7


def test_sparse_entry_rejects_invalid_arguments():
    from pinsage_hip import native
    if not native.have_lib():
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(native.SO_PATH)
    lib.ps_cooc_pairs_sparse_workspace_bytes.restype = ctypes.c_size_t
    i64, i32, p, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    one = p(256)      # never dereferenced: every call below returns before any device work
    h = ctypes.c_int64(0)
    wsb = lib.ps_cooc_pairs_sparse_workspace_bytes
    need = wsb(i64(40), i32(0))
    # O(M) and a bounded number of M-long slabs (12 bytes per item): at most 512 of them, at most 2 GiB, at least 4
    assert 0 < need <= 512 + 4 * 40 + 512 * 12 * 40
    for M in (10 ** 6, 10 ** 8, 10 ** 9):
        assert 12 * M <= wsb(i64(M), i32(8)) <= 512 + 4 * M + max(2 << 30, 4 * 12 * M)
    assert wsb(i64(0), i32(0)) == 0 and wsb(i64(1 << 31), i32(0)) == 0
    assert wsb(i64(40), i32(-1)) == 0 and wsb(i64(40), i32(1 << 20)) == 0

    def sp(n=10, U=100, M=40, max_sq=100, thr=1, slots=0, rec=one, cap=10, count=one, hc=ctypes.byref(h), ws=one, wsn=need,
           iptr=one, iuser=one, eptr=one, eitem=one, order=one):
        return lib.ps_cooc_pairs_sparse(iptr, iuser, one, eptr, eitem, one, order, i64(n), i64(U), i64(M), i64(max_sq), i64(thr),
                                        i32(slots), rec, i64(cap), count, hc, ws, sz(wsn), p(0))

    assert sp(thr=0) == native.PS_EINVAL
    assert sp(n=-1) == native.PS_EINVAL
    assert sp(U=0) == native.PS_EINVAL and sp(U=1 << 31) == native.PS_EINVAL
    assert sp(M=0) == native.PS_EINVAL and sp(M=1 << 31) == native.PS_EINVAL
    assert sp(cap=-1) == native.PS_EINVAL and sp(max_sq=-1) == native.PS_EINVAL
    assert sp(slots=-1) == native.PS_EINVAL and sp(slots=1 << 20) == native.PS_EINVAL
    assert sp(max_sq=1 << 31) == native.PS_EUNSUPPORTED
    assert sp(max_sq=(1 << 31) - 1, wsn=0) == native.PS_EWORKSPACE          # 2^31 - 1 is in range
    for null in ("iptr", "iuser", "eptr", "eitem", "order", "rec", "count", "hc", "ws"):
        assert sp(**{null: p(0)}) == native.PS_EINVAL, null
    assert sp(ws=p(260)) == native.PS_EINVAL                                # workspace not 8-byte aligned
    assert sp(wsn=need - 1) == native.PS_EWORKSPACE


def test_unknown_method_raises():
    from pinsage_hip import cooc
    with pytest.raises(ValueError, match="bogus"):
        cooc.item_cooccurrence_graph(torch.tensor([1, 1]), torch.tensor([0, 1]), 2, method="bogus")
    assert cooc.METHODS == ("dense", "sparse", "auto")
    import inspect
    sig = inspect.signature(cooc.item_cooccurrence_graph)
    assert sig.parameters["method"].default == "dense" and sig.parameters["acc_slots"].default == 0
    from data.graph_builder import GraphBuilder
    assert GraphBuilder.cooc_method == "auto"


# ---------------------------------------------------------------------------------------------------------- GPU

def _graph(case, thr, **kw):
    return _graph_of(*cases.rows(case), thr, **kw)


def _graph_of(users, items, M, thr, **kw):
    from pinsage_hip import cooc
    ei, ew = cooc.item_cooccurrence_graph(torch.from_numpy(np.array(users, np.int64)), torch.from_numpy(np.array(items, np.int64)),
                                          M, threshold=thr, device="cuda", **kw)
    assert ei.dtype == torch.int64 and ew.dtype == torch.float32
    return ei.cpu().numpy(), ew.cpu().numpy()


def _same(got, want):
    return got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


class _Dataset:
    def __init__(self, df, user_map, movie_map):
        self.ratings_df = df
        self.user_id_to_idx = user_map
        self.movie_id_to_idx = movie_map


@pytest.mark.gpu
def test_sparse_drop_in_matches_golden(capsys, monkeypatch):
    import pandas as pd
    from data.graph_builder import GraphBuilder
    from pinsage_hip import native
    lib = native.lib()
    real, calls = lib.ps_cooc_pairs_sparse, []
    monkeypatch.setattr(lib, "ps_cooc_pairs_sparse", lambda *a: calls.append(1) or real(*a))
    gold = np.load(GOLDEN)
    for f in range(3):
        df = pd.DataFrame({"userId": gold[f"f{f}_user"], "movieId": gold[f"f{f}_movie"], "rating": gold[f"f{f}_rating"],
                           "timestamp": np.arange(gold[f"f{f}_user"].size)})
        ds = _Dataset(df, {int(k): int(v) for k, v in gold[f"f{f}_umap"]}, {int(k): int(v) for k, v in gold[f"f{f}_mmap"]})
        for t in THRESHOLDS:
            gb = GraphBuilder(ds)
            gb.cooc_method = "sparse"
            capsys.readouterr()
            ei, ew = gb.build_item_similarity_graph(threshold=t)
            tag = f"f{f}_t{t}"
            assert capsys.readouterr().out == str(gold[f"{tag}_out"]), tag
            assert ei.device.type == "cpu" and ew.device.type == "cpu"
            assert ei.dtype == torch.int64 and ew.dtype == torch.float32
            assert _same((ei.numpy(), ew.numpy()), (gold[f"{tag}_ei"], gold[f"{tag}_ew"])), tag
            assert gb.edge_index is None and gb.edge_weight is None
    assert len(calls) == 3 * len(THRESHOLDS)                 # every graph came from the sparse producer


@pytest.mark.gpu
@pytest.mark.parametrize("U,M,R,maxm,thr", cases.SHAPES)
def test_sparse_equals_restatement_equals_dense(U, M, R, maxm, thr):
    case = ("shape", U, M, R, maxm)
    want = cases.restated(case, thr)
    sparse = _graph(case, thr, method="sparse")
    assert _same(sparse, want)
    assert _same(_graph(case, thr, method="dense"), sparse)
    if thr <= 1:
        pairs = set(zip(sparse[0][0, 0::2].tolist(), sparse[0][1, 0::2].tolist()))
        assert set(cases.planted_pairs(U, M)) <= pairs


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [16, 64])
def test_mixed_hash_direct_and_slab_rows(slots):
    """200 items against 16 / 64 slots: rows whose partners fit are done in the hash, the others fail it and are redone in a
    global slab, the last rows are direct-indexed"""
    case = ("shape", 1037, 200, 3000, 3)
    assert _same(_graph(case, 1, method="sparse", acc_slots=slots), cases.restated(case, 1))


@pytest.mark.gpu
def test_more_items_than_default_slots():
    assert _same(_graph(WIDE, 1, method="sparse"), cases.restated(WIDE, 1))


@pytest.mark.gpu
def test_accumulator_overflow_is_exact():
    want = cases.restated(("overflow",), 1)
    got = [_graph(("overflow",), 1, method="sparse", acc_slots=s) for s in cases.OVERFLOW_SLOTS]
    for s, g in zip(cases.OVERFLOW_SLOTS, got):
        assert _same(g, want), s
        assert _same(g, got[0]), s


@pytest.mark.gpu
def test_beyond_the_dense_limits():
    for case in (("beyond",), ("m128",)):
        want = cases.restated(case, 1)
        assert _same(_graph(case, 1, method="sparse"), want), case
        assert _same(_graph(case, 1, method="auto"), want), case
        with pytest.raises(ValueError):
            _graph(case, 1, method="dense")
    ei, ew = _graph(("beyond",), 1, method="sparse")
    w = {(int(a), int(b)): float(x) for a, b, x in zip(ei[0, 0::2], ei[1, 0::2], ew[0::2])}
    assert w[(2, 5)] == 16801802.0 and w[(2, 7)] == float(np.float32(4099 * 4097)) and w[(2, 2)] == 4099 * 4098 / 2
    # a threshold between the two large counts is compared with the exact integer, not the rounded weight
    ei, ew = _graph(("beyond",), 4099 * 4097 + 1, method="sparse")
    assert ei.tolist() == [[2, 5], [5, 2]] and ew.tolist() == [16801802.0] * 2


@pytest.mark.gpu
def test_auto_routing(monkeypatch):
    from pinsage_hip import cooc, native
    lib = native.lib()
    calls = {"sparse": 0, "dense": 0}
    real_sparse, real_dense = lib.ps_cooc_pairs_sparse, lib.ps_cooc_pairs

    def sparse(*a):
        calls["sparse"] += 1
        return real_sparse(*a)

    def dense(*a):
        calls["dense"] += 1
        return real_dense(*a)

    monkeypatch.setattr(lib, "ps_cooc_pairs_sparse", sparse)
    monkeypatch.setattr(lib, "ps_cooc_pairs", dense)
    U, M, R, maxm, thr = cases.SHAPES[2]
    case = ("shape", U, M, R, maxm)
    want = cases.restated(case, thr)
    assert _same(_graph(case, thr, method="auto"), want) and calls == {"sparse": 0, "dense": 1}
    seen = []
    monkeypatch.setattr(cooc, "_dense_fits", lambda nbytes, device: seen.append(nbytes) or False)
    assert _same(_graph(case, thr, method="auto"), want) and calls == {"sparse": 1, "dense": 1}
    assert seen == [lib.ps_cooc_planes_bytes(ctypes.c_int64(U), ctypes.c_int64(M), ctypes.c_int(maxm))]
    assert _same(_graph(case, thr), want) and calls == {"sparse": 1, "dense": 2}          # the default stays dense


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 7])
def test_sparse_small_capacity_reruns(cap):
    assert _same(_graph(("rerun",), 1, method="sparse", capacity=cap), cases.restated(("rerun",), 1))


@pytest.mark.gpu
def test_sparse_empty_and_trivial_inputs():
    for method in ("sparse", "auto"):
        ei, ew = _graph_of(np.zeros(0, np.int64), np.zeros(0, np.int64), 5, 1, method=method)
        assert ei.shape == (2, 0) and ew.shape == (0,)
        ei, ew = _graph_of([1, 2, 3], [0, 1, 2], 5, 1, method=method)            # nobody rates two items
        assert ei.shape == (2, 0) and ew.shape == (0,)
        ei, ew = _graph_of([9, 9], [4, 4], 5, 1, method=method)                  # one self pair
        assert ei.tolist() == [[4, 4], [4, 4]] and ew.tolist() == [1.0, 1.0]
        for thr in (10 ** 6, 2.0 ** 40, float("nan"), float("inf"), 1e30):      # above every count / no count can pass
            ei, ew = _graph(("overflow",), thr, method=method)
            assert ei.shape == (2, 0) and ew.shape == (0,), thr
    ei, ew = _graph(("overflow",), -3, method="sparse")                          # a threshold below 1 keeps every pair
    assert _same((ei, ew), cases.restated(("overflow",), 1))


@pytest.mark.gpu
def test_sparse_graph_feeds_sampler_like_dense():
    from utils.random_walk import RandomWalkSampler
    case = ("sampler",)
    sparse, dense = _graph(case, 3, method="sparse"), _graph(case, 3, method="dense")
    assert _same(sparse, dense) and _same(sparse, cases.restated(case, 3)) and sparse[1].size > 0
    nodes = np.unique(sparse[0][0])
    out = []
    for ei, ew in (sparse, dense):
        s = RandomWalkSampler(torch.from_numpy(ei.copy()), torch.from_numpy(ew.copy()), walk_length=2, num_walks=20, rng="numpy")
        np.random.seed(42)
        b = s.sample_batch(nodes, 10)
        out.append((b.ids.cpu().numpy(), b.counts.cpu().numpy(), b.nvalid.cpu().numpy()))
    assert all(np.array_equal(x, y) for x, y in zip(*out))
