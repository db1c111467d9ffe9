"""Personalized-PageRank neighbourhoods on the device (csrc/ppr_push.hip, pinsage_hip/ppr.py, RandomWalkSampler's PPR methods)
against the reference's recorded outputs (tests/golden/reference_golden_ppr.npz): fp64 scores and weights bit for bit, ids in
the same order.  One caveat: for a source >= V the unmodified reference raises IndexError (utils/random_walk.py:180); those
rows were recorded from the reference with its adjacency list padded by empty rows (tests/golden/make_golden_ppr.py), i.e. with
such a source as a node without edges.  The cases and the restated arithmetic are tests/helpers/ppr_cases.py;
tests/test_ppr_cases.py holds both to the fixture without a GPU."""
import ctypes
import functools
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ppr_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _sampler(name):
    from utils.random_walk import RandomWalkSampler
    ei, ew = pc.case(name)[:2]
    return RandomWalkSampler(torch.from_numpy(ei.copy()), torch.from_numpy(ew.copy()), walk_length=2, num_walks=10)


def _bits(alpha):
    return struct.unpack("<Q", struct.pack("<d", alpha))[0]


@pytest.mark.parametrize("name", pc.NAMES)
def test_scores_equal_the_reference(name):
    from pinsage_hip import ppr
    g = pc.golden()
    _, _, sources, alpha, sweeps, _ = pc.case(name)
    got = ppr.ppr_scores(_sampler(name).graph, list(sources), alpha, sweeps)
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), g[f"{name}_scores"])


def test_level_lists():
    from pinsage_hip import ppr
    for name in ("bip10", "chain", "random"):
        pg = ppr.ppr_graph(_sampler(name).graph)
        lev = np.array(pc.levels(pc.adjacency(name), pc.num_nodes(name)))
        assert pg.n_levels == lev.max() + 1 == {"bip10": 2, "chain": 48}.get(name, pg.n_levels)
        nodes = pg.level_nodes.cpu().numpy()
        assert np.array_equal(nodes, np.argsort(lev, kind="stable")) and list(pg.level_ptr) == [0] + list(np.cumsum(np.bincount(lev)))


def _bip_sources(n):
    """n sources drawn over the recorded ones of bip10 (every node and one id beyond the graph), and their fixture rows"""
    pick = (np.arange(n) * 7 + 3) % len(pc.case("bip10")[2])
    return [pc.case("bip10")[2][i] for i in pick], pc.golden()["bip10_scores"][pick]


@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_source_counts_and_chunkings(n):
    """one slab with idle lanes, one slab short of full, two slabs, and 130 sources in one chunk and in three (64 + 64 + 2)"""
    from pinsage_hip import ppr
    graph = _sampler("bip10").graph
    sources, want = _bip_sources(n)
    width = max(graph.V, max(sources) + 1)
    assert not want[:, width:].any()
    got = ppr.ppr_scores(graph, sources, 0.15, 10)
    assert tuple(got.shape) == (n, width) and np.array_equal(got.cpu().numpy(), want[:, :width])
    if n == 130:
        split = ppr.ppr_scores(graph, sources, 0.15, 10, source_chunk=64)
        assert torch.equal(split, got)
        top, top_split = ppr.ppr_topk(graph, sources, 5), ppr.ppr_topk(graph, sources, 5, source_chunk=64)
        assert torch.equal(top.ids, top_split.ids) and torch.equal(top.wts, top_split.wts) and torch.equal(top.nvalid, top_split.nvalid)


def test_state_byte_offsets_beyond_2_32():
    """1 024 source columns and a source id of 2^19 + 8 put the last rows of the node-major state, and of the source-major
    copy the cut reads, past byte 2^32 (element 2^29): the offsets a 32-bit index would wrap.  The rows of the graph's own
    sources stay the recorded ones, the far source holds 1 + alpha at itself and nothing else, and nothing is written anywhere
    else.  The state, its two push buffers and the copy are 4.3 GB each; the test fails with a plain message, instead of an
    allocator error, where 24 GB are not free.  (Element 2^31 would take four buffers of 17 GB; every offset in
    csrc/ppr_push.hip is computed in int64.)"""
    from pinsage_hip import ppr
    g = pc.golden()
    graph = _sampler("stars").graph
    far = (1 << 19) + 8
    sources = [0] * 1022 + [17, far]
    assert (far + 1) * 1024 * 8 > 2 ** 32
    free = torch.cuda.mem_get_info(graph.device)[0]
    assert free >= 24 << 30, f"this test needs 24 GB of free device memory, {free >> 30} GB are free"
    got = ppr.ppr_scores(graph, sources, 0.15, 10, source_chunk=1024)
    assert tuple(got.shape) == (1024, far + 1) and got.is_contiguous()
    V = graph.V
    near = got[:, :V].cpu().numpy()
    want = g["stars_scores"][:, :V]
    assert np.array_equal(near[0], want[0]) and np.array_equal(near[1021], want[0]) and np.array_equal(near[1022], want[1])
    assert not near[1023].any()
    assert torch.count_nonzero(got).item() == np.count_nonzero(near) + 1 and got[1023, far].item() == 1.0 + 0.15 * 1.0
    del got
    top = ppr.ppr_topk(graph, sources, 2, source_chunk=1024)
    assert top.ids[1023].tolist() == [far, -1] and top.wts[1023].tolist() == [1.0, 0.0] and top.nvalid[1023].item() == 1
    assert top.ids[1022].tolist() == [int(t) for t in g["stars_top_ids"][1, :2]] and top.nvalid[1022].item() == 2


def test_row_skipping_changes_nothing():
    from pinsage_hip import ppr
    for name in ("hub", "random"):
        _, _, sources, alpha, sweeps, _ = pc.case(name)
        graph = _sampler(name).graph
        assert torch.equal(ppr.ppr_scores(graph, list(sources), alpha, sweeps, skip_rows=False),
                           ppr.ppr_scores(graph, list(sources), alpha, sweeps))


@pytest.mark.parametrize("name", pc.NAMES)
def test_shares_equal_the_left_to_right_quotients(name):
    from pinsage_hip import ppr
    want = [s for row in pc.shares(pc.adjacency(name)) for s in row]
    assert np.array_equal(ppr.ppr_graph(_sampler(name).graph).share.cpu().numpy(), np.array(want, dtype=np.float64))


@pytest.mark.parametrize("name", pc.NAMES)
def test_top_neighbours_equal_the_reference(name):
    from pinsage_hip import ppr
    g = pc.golden()
    _, _, sources, _, _, k = pc.case(name)
    s = _sampler(name)
    ids, w, nvalid = g[f"{name}_top_ids"], g[f"{name}_top_w"], g[f"{name}_top_nvalid"]
    batch = ppr.ppr_topk(s.graph, list(sources), k)                      # alpha 0.15, 10 sweeps: what the reference's method runs
    assert batch.ids.dtype == torch.int32 and batch.wts.dtype == torch.float64 and (batch.B, batch.T) == (len(sources), k)
    assert np.array_equal(batch.ids.cpu().numpy(), ids) and np.array_equal(batch.wts.cpu().numpy(), w)
    assert np.array_equal(batch.nvalid.cpu().numpy(), nvalid)
    top = s.precompute_top_neighbors(list(sources), num_neighbors=k)
    assert list(top) == list(dict.fromkeys(sources))
    for i, src in enumerate(sources):
        a, b = top[src]
        assert a == [int(t) for t in ids[i, :nvalid[i]]] and all(type(t) is int for t in a)
        assert b == [float(v) for v in w[i, :nvalid[i]]] and all(type(v) is float for v in b)
    nb, wt = batch.to_lists()
    assert all(isinstance(t, np.int64) for row in nb for t in row) and all(type(v) is float for row in wt for v in row)
    assert [[int(t) for t in row] for row in nb] == [top[src][0] for src in sources] and wt == [top[src][1] for src in sources]


def test_max_target_keeps_the_items():
    """only ids below max_target compete: the cut of the recorded score rows restricted to the items"""
    g = pc.golden()
    sources = list(pc.case("bip10")[2])
    batch = _sampler("bip10").ppr_batch(sources, num_neighbors=6, max_target=pc.BIP_M)
    nb, wt = batch.to_lists()
    for i in range(len(sources)):
        ids, w = pc.select(g["bip10_scores"][i], 6, max_target=pc.BIP_M)
        assert [int(t) for t in nb[i]] == ids and wt[i] == w and max(ids, default=0) < pc.BIP_M
    assert batch.nvalid[-1].item() == 0 and (batch.ids[-1] == -1).all()   # the source beyond the graph reaches no item


@pytest.mark.parametrize("name", ["bip4", "random", "stars"])
def test_ppr_matrix_dict(name):
    g = pc.golden()
    _, _, sources, alpha, sweeps, _ = pc.case(name)
    got = _sampler(name).compute_ppr_matrix(list(sources), alpha=alpha, num_iterations=sweeps)
    want = {}
    for i, src in enumerate(sources):
        want.update({(src, int(t)): float(g[f"{name}_scores"][i, t]) for t in np.flatnonzero(g[f"{name}_scores"][i] > 0)})
    assert list(got) == list(want) and list(got.values()) == list(want.values())
    assert all(type(a) is int and type(b) is int for a, b in got) and all(type(v) is float for v in got.values())
    from_tensor = _sampler(name).compute_ppr_matrix(torch.tensor(sources), alpha=alpha, num_iterations=sweeps)
    assert list(from_tensor.items()) == list(got.items())


@pytest.mark.parametrize("name", ["bip4", "chain", "random", "hub"])
def test_host_and_device_methods_agree(name, monkeypatch):
    from utils.random_walk import RandomWalkSampler
    assert RandomWalkSampler.ppr_method == "device"
    _, _, sources, alpha, sweeps, k = pc.case(name)
    s = _sampler(name)
    dev = s.compute_ppr_matrix(list(sources), alpha=alpha, num_iterations=sweeps)
    dev_top = s.precompute_top_neighbors(list(sources), num_neighbors=k)
    monkeypatch.setattr(RandomWalkSampler, "ppr_method", "host")
    host = s.compute_ppr_matrix(list(sources), alpha=alpha, num_iterations=sweeps)
    host_top = s.precompute_top_neighbors(list(sources), num_neighbors=k)
    assert list(host.items()) == list(dev.items()) and list(host_top.items()) == list(dev_top.items())
    monkeypatch.setattr(RandomWalkSampler, "ppr_method", "neither")
    with pytest.raises(ValueError):
        s.compute_ppr_matrix([0])


def test_pooling_and_forward_take_a_weighted_batch():
    from model.pinsage import ImportancePooling, PinSage
    from pinsage_hip import sampling
    s = _sampler("bip10")
    n = pc.BIP_M + pc.BIP_U
    batch = s.ppr_batch(list(range(n)), num_neighbors=10)
    assert isinstance(batch, sampling.WeightedBatch) and (batch.B, batch.T) == (n, 10)
    nb, wt = batch.to_lists()
    torch.manual_seed(5)
    x = torch.randn(n, 24, device="cuda")
    lazy = sampling.LazyNeighborList(batch, "ids"), sampling.LazyNeighborList(batch, "weights")
    assert lazy[0] == nb and lazy[1] == wt
    pool = ImportancePooling().eval()
    model = PinSage(24, 32, 16, num_layers=2).cuda().eval()
    with torch.no_grad():
        want = pool(x, nb, wt)
        assert want.abs().sum().item() > 0
        assert torch.equal(pool(x, batch, None), want) and torch.equal(pool(x, *lazy), want)
        emb = model(x, sampled_neighbors=[nb, nb], importance_weights=[wt, wt])      # one (neighbors, weights) pair per layer
        assert emb.abs().sum().item() > 0
        assert torch.equal(model(x, sampled_neighbors=[lazy[0], lazy[0]], importance_weights=[lazy[1], lazy[1]]), emb)
        assert torch.equal(model(x, sampled_neighbors=batch, importance_weights=batch), emb)


def test_two_runs_are_bit_identical():
    from pinsage_hip import ppr
    _, _, sources, alpha, sweeps, k = pc.case("hub")
    graph = _sampler("hub").graph
    a, b = ppr.ppr_scores(graph, list(sources), alpha, sweeps), ppr.ppr_scores(graph, list(sources), alpha, sweeps)
    assert torch.equal(a, b)
    ta, tb = ppr.ppr_topk(graph, list(sources), k), ppr.ppr_topk(graph, list(sources), k)
    assert torch.equal(ta.ids, tb.ids) and torch.equal(ta.wts, tb.wts) and torch.equal(ta.scores, tb.scores)


def test_bad_arguments_are_refused():
    from pinsage_hip import native as nv
    from pinsage_hip import ppr
    lib = nv.lib()
    graph = _sampler("stars").graph
    pg = ppr.ppr_graph(graph)
    V, S = pg.V, 3
    src = torch.tensor([0, 1, 2], dtype=torch.int64, device="cuda")
    score = torch.zeros((V, 64), dtype=torch.float64, device="cuda")
    ws, wsb = nv.workspace("ps_ppr_push_workspace_bytes", graph.device, V, S)
    assert wsb > 0 and lib.ps_ppr_push_workspace_bytes(-1, 3) == 0 and lib.ps_ppr_push_workspace_bytes(V, -3) == 0

    def push(V=V, Vp=V, S=S, alpha=0.15, sweeps=2, flags=0, wsb=wsb, n_levels=pg.n_levels):
        return lib.ps_ppr_push(nv.ptr(pg.in_rowptr), nv.ptr(pg.in_src), nv.ptr(pg.in_share), V, Vp, nv.ptr(pg.level_nodes),
                               pg.level_ptr.ctypes.data, n_levels, nv.ptr(src), S, _bits(alpha), sweeps, flags, nv.ptr(score),
                               nv.ptr(ws), wsb, nv.stream())

    assert push() == nv.PS_OK
    for bad in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=-0.15), dict(alpha=1.5), dict(alpha=float("nan")), dict(S=-1),
                dict(V=-1), dict(Vp=V - 1), dict(sweeps=-1), dict(n_levels=-1), dict(flags=2), dict(wsb=wsb - 1), dict(wsb=0)):
        assert push(**bad) == nv.PS_EINVAL, bad
    rows = torch.zeros((S, V), dtype=torch.float64, device="cuda")
    ids = torch.empty((S, 4), dtype=torch.int32, device="cuda")
    sc, wt = torch.empty((S, 4), dtype=torch.float64, device="cuda"), torch.empty((S, 4), dtype=torch.float64, device="cuda")
    nvalid = torch.empty(S, dtype=torch.int32, device="cuda")

    def topk(S=S, ld=V, Vp=V, k=4):
        return lib.ps_ppr_topk(nv.ptr(rows), S, ld, Vp, -1, k, nv.ptr(ids), nv.ptr(sc), nv.ptr(wt), nv.ptr(nvalid), nv.stream())

    assert topk() == nv.PS_OK
    for bad in (dict(k=0), dict(k=-2), dict(S=-1), dict(Vp=-1), dict(ld=V - 1)):
        assert topk(**bad) == nv.PS_EINVAL, bad
    assert lib.ps_ppr_shares(nv.ptr(graph.rowptr), nv.ptr(graph.wsorted), -1, nv.ptr(pg.share), nv.stream()) == nv.PS_EINVAL
    torch.cuda.synchronize()
    assert (nvalid == 0).all() and (ids == -1).all()                      # all-zero rows: nothing is positive
    with pytest.raises(ctypes.ArgumentError):
        lib.ps_ppr_push(nv.ptr(pg.in_rowptr), nv.ptr(pg.in_src), nv.ptr(pg.in_share), V, V, nv.ptr(pg.level_nodes),
                        pg.level_ptr.ctypes.data, pg.n_levels, nv.ptr(src), S, 0.15, 2, 0, nv.ptr(score), nv.ptr(ws), wsb, nv.stream())
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(sweeps=-1), dict(source_chunk=100)):
        with pytest.raises(ValueError):
            ppr.ppr_scores(graph, [0, 1], **kw)
    with pytest.raises(ValueError):
        ppr.ppr_topk(graph, [0, 1], 0)
