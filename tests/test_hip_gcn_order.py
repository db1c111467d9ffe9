"""ps_gcn_order (the row order of all layers in one launch) word for word against its numpy restatement, ps_gcn_layer_ordered against
ps_gcn_layer and against the pair both replace, and one ShardedPinSage.embed with the hoisted order against one without it."""
import functools

import numpy as np
import pytest
import torch

from helpers import gcn_cases as gn
from helpers import gcn_order as go

pytestmark = pytest.mark.gpu

T, K, H = 10, 32, 64


@functools.lru_cache(maxsize=None)
def _rows(M):
    """per pattern the planted rows (ids, counts, nvalid; tests/helpers/gcn_cases.make_rows: ids equal to max_idx are kept, ids
    equal to max_idx + 1 dropped, -1 pads, nvalid below and above T) and the restated order; h_full has M + 50 rows, max_idx
    leaves its last 40 out of reach"""
    n_full = M + 50
    max_idx = n_full - 41
    out = []
    for name in go.PATTERNS:
        keeps = go.pattern(name, M)
        rows = gn.make_rows(keeps, T, max_idx, n_full + 9, np.random.RandomState(gn._seed(f"{name}-{M}")))
        assert np.array_equal(gn.row_keeps(rows.ids, rows.nvalid, T, max_idx), keeps)
        if name == "random":                              # the bound itself: kept at max_idx, dropped one above it
            assert (rows.ids == max_idx).any() and (rows.ids == max_idx + 1).any()
        out.append((name, rows, go.chunk_partition(keeps)))
    return n_full, max_idx, out


def _order(ids, nvalid, max_idx):
    from pinsage_hip import native as nv
    layers, M = nvalid.shape
    ntiles = -(-M // 64)
    ord_ = torch.full((layers, ntiles * 64), -7, dtype=torch.int32, device=ids.device)
    heavy = torch.full((layers, ntiles), -7, dtype=torch.int32, device=ids.device)
    rc = nv.lib().ps_gcn_order(nv.ptr(ids), nv.ptr(nvalid), layers, M, ids.size(2), max_idx, nv.ptr(ord_), nv.ptr(heavy), nv.stream())
    assert rc == nv.PS_OK, rc
    return ord_, heavy


@pytest.mark.parametrize("M", go.SIZES)
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_order_equals_the_restatement(M, layers):
    n_full, max_idx, pats = _rows(M)
    dev = torch.device("cuda")
    starts = list(range(0, len(pats) - layers + 1, layers))
    if starts[-1] != len(pats) - layers:
        starts.append(len(pats) - layers)
    for s in starts:                                       # every pattern, `layers` of them per launch
        grp = pats[s:s + layers]
        ids = torch.from_numpy(np.stack([r.ids for _, r, _ in grp])).to(dev)
        nvalid = torch.from_numpy(np.stack([r.nvalid for _, r, _ in grp])).to(dev)
        ord_, heavy = _order(ids, nvalid, max_idx)
        for j, (name, _, (ord_ref, heavy_ref)) in enumerate(grp):
            assert np.array_equal(ord_[j].cpu().numpy(), ord_ref), (name, j)
            assert np.array_equal(heavy[j].cpu().numpy(), heavy_ref), (name, j)


def _layer_args(M):
    g = torch.Generator(device="cpu").manual_seed(M)
    dev = torch.device("cuda")
    n_full = M + 50
    x, h_full = torch.randn(M, K, generator=g), torch.randn(n_full, H, generator=g)
    W, W2, b = torch.randn(256, K, generator=g) * 0.1, torch.randn(256, H, generator=g) * 0.1, torch.randn(256, generator=g) * 0.1
    return [t.to(dev).contiguous() for t in (x, h_full, W, W2, b)]


def _same(a, b, what):
    assert torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32)), what


@pytest.mark.parametrize("M", go.SIZES)
def test_ordered_layer_equals_the_layer_and_the_pair(M):
    from pinsage_hip import dense, sampling
    from pinsage_hip import native as nv
    n_full, max_idx, pats = _rows(M)
    x, h_full, W, W2, b = _layer_args(M)
    dev = x.device
    L = nv.lib()
    wsb = int(L.ps_gcn_layer_workspace_bytes(M, H))
    flags = nv.PS_RELU | nv.PS_L2NORM
    for name, rows, _ in pats:
        ids, counts, nvalid = (torch.from_numpy(a).to(dev) for a in (rows.ids, rows.counts, rows.nvalid))
        ord_, heavy = _order(ids[None], nvalid[None], max_idx)
        out = []
        for ordered in (True, False):
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            y = torch.full((M, 256), float("nan"), device=dev)
            args = (nv.ptr(x), M, K, nv.ptr(W), K, nv.ptr(b), 256, nv.ptr(h_full), n_full, H, nv.ptr(ids), nv.ptr(counts), None,
                    nv.ptr(nvalid), T, max_idx, 1, nv.ptr(W2), H, flags, nv.ptr(y), nv.ptr(ws), wsb)
            rc = L.ps_gcn_layer_ordered(*args, nv.ptr(ord_), nv.ptr(heavy), nv.stream()) if ordered else L.ps_gcn_layer(*args, nv.stream())
            assert rc == nv.PS_OK, (name, ordered, rc)
            out.append(y)
        pooled = sampling.importance_pool(h_full, ids=ids, counts=counts, nvalid=nvalid, max_idx=max_idx, renorm=True)
        pair = dense.linear(x, W, b, x2=pooled, W2=W2, relu=True, l2norm=True)
        _same(out[0], out[1], f"{name}: ps_gcn_layer_ordered != ps_gcn_layer")
        _same(out[0], pair, f"{name}: ps_gcn_layer_ordered != importance_pool + linear")
        got = dense.gcn_layer(x, W, b, h_full, ids, counts, nvalid, W2, max_idx=max_idx, order=(ord_[0], heavy[0]))
        _same(got, pair, f"{name}: dense.gcn_layer(order=...)")


def test_orders_of_sampled_slices_and_of_separate_tensors():
    """dense.gcn_orders takes consecutive slices of one buffer as that buffer and stacks anything else: the same orders"""
    from pinsage_hip import dense
    M = go.SIZES[1]
    n_full, max_idx, pats = _rows(M)
    dev = torch.device("cuda")
    ids = torch.from_numpy(np.stack([r.ids for _, r, _ in pats[-3:]])).to(dev)
    nvalid = torch.from_numpy(np.stack([r.nvalid for _, r, _ in pats[-3:]])).to(dev)
    a = dense.gcn_orders([ids[r] for r in range(3)], [nvalid[r] for r in range(3)], max_idx)
    b = dense.gcn_orders([ids[r].clone() for r in (0, 1, 2)], [nvalid[r].clone() for r in (0, 1, 2)], max_idx)
    for j, (name, _, (ord_ref, heavy_ref)) in enumerate(pats[-3:]):
        for o, h in (a[j], b[j]):
            assert np.array_equal(o.cpu().numpy(), ord_ref) and np.array_equal(h.cpu().numpy(), heavy_ref), name
    assert dense.gcn_orders([ids[0][:1000]], [nvalid[0][:1000]], max_idx) is None          # below the layer's gate: no order


def test_embed_with_the_hoisted_order_equals_embed_without():
    from pinsage_hip import synth
    from pinsage_hip.graph import DeviceGraph
    from pinsage_hip.shard import HipOps, ShardedPinSage
    from utils.random_walk import RandomWalkSampler
    from model.pinsage import PinSage
    dev = torch.device("cuda")
    M = go.SIZES[2]
    ei, ew = synth.bipartite_ratings(3000, M, 400_000, seed=8, device=dev)
    sampler = RandomWalkSampler.from_graph(DeviceGraph(ei, ew, device=dev), walk_length=2, num_walks=100, rng="philox", seed=42)
    torch.manual_seed(3)
    model = PinSage(32, 256, 64, 2).to(dev).eval()
    P = {k: v.detach().float().contiguous() for k, v in model.state_dict().items()}
    x = torch.randn(M, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    class Counting(HipOps):
        made = 0

        def gcn_orders(self, batches, max_idx):
            orders = super().gcn_orders(batches, max_idx)
            Counting.made += orders is not None
            return orders

    class PerLayer:                                        # a backend without gcn_orders: every layer call makes its own order
        def __init__(self):
            self._ops = HipOps()

        def __getattr__(self, name):
            if name == "gcn_orders":
                raise AttributeError(name)
            return getattr(self._ops, name)

    out = []
    for ops in (Counting(), PerLayer()):
        sampler._calls = 0
        out.append(ShardedPinSage(P, 2, sampler, M, ops=ops).embed(x, T))
    assert Counting.made == 1 and not hasattr(PerLayer(), "gcn_orders")
    _same(out[0], out[1], "embed with gcn_orders != embed without")
    assert torch.isfinite(out[0]).all() and out[0].abs().sum() > 0
