"""ps_gcn_layer (pooling inside the layer GEMM, rows that keep no neighbour skip the W2 half) against the pair it replaces,
ps_importance_pool + ps_linear: torch.equal everywhere -- on the SYN-25M batches of the benchmark (both layers, T = 10 through
ps_gcn_layer, T = 50 through the pair dense.gcn_layer falls back to),
on synthetic batches around the edges of the row classification, and end to end through ShardedPinSage.embed with
PS_GCN_FUSED=0 against the default."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 64 * 384 + 37                     # the smallest row count the fused path serves, plus a partial last tile


def _pair(x, W, b, h_full, ids, counts, wts, nvalid, W2, max_idx, renorm):
    from pinsage_hip import dense, sampling
    h = sampling.importance_pool(h_full, ids=ids, counts=counts, wts=wts, nvalid=nvalid, max_idx=max_idx, renorm=renorm)
    return dense.linear(x, W, b, x2=h, W2=W2, relu=True, l2norm=True)


def _fused(x, W, b, h_full, ids, counts, wts, nvalid, W2, max_idx, renorm):
    """ps_gcn_layer itself: fails if the call is not served (no silent fall-back to the pair)"""
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    staged = isinstance(W, dense.StagedWeight)
    Wm, W2m = (W.t, W2.t) if staged else (W, W2)
    M, K = x.shape
    n_full, H = h_full.shape
    T = ids.size(1)
    L = nv.lib()
    wsb = int(L.ps_gcn_layer_workspace_bytes(nv.i64(M), nv.i32(H)))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    y = torch.full((M, Wm.size(0)), float("nan"), device=x.device)
    flags = nv.PS_RELU | nv.PS_L2NORM | (nv.PS_WPERM if staged else 0)
    rc = L.ps_gcn_layer(nv.ptr(x), nv.i64(M), nv.i32(K), nv.ptr(Wm), nv.i32(Wm.stride(0)), nv.ptr(b), nv.i32(Wm.size(0)),
                        nv.ptr(h_full), nv.i64(n_full), nv.i32(H), nv.ptr(ids), nv.ptr(counts), nv.ptr(wts), nv.ptr(nvalid),
                        nv.i32(T), nv.i64(max_idx), nv.i32(renorm), nv.ptr(W2m), nv.i32(W2m.stride(0)), nv.i32(flags), nv.ptr(y),
                        nv.ptr(ws), nv.C.c_size_t(wsb), nv.stream())
    assert rc == nv.PS_OK, rc
    return y


def _same(a, b):
    assert torch.equal(a, b), f"{(a != b).sum().item()} of {a.numel()} differ"
    # torch.equal treats -0.0 == +0.0: the bits too
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _heavy_fraction(ids, nvalid, max_idx):
    T = ids.size(1)
    slot = torch.arange(T, device=ids.device)[None, :]
    kept = (slot < nvalid[:, None]) & (ids >= 0) & (ids <= max_idx)
    return kept.any(dim=1).float().mean().item()


@pytest.fixture(scope="module")
def syn25m():
    from pinsage_hip import synth
    from pinsage_hip.graph import DeviceGraph
    from utils.random_walk import RandomWalkSampler
    from model.pinsage import PinSage
    dev = torch.device("cuda")
    src = synth.ML25M
    M = src["num_items"]
    ei, ew = synth.bipartite_ratings(src["num_users"], M, src["num_ratings"], seed=20240601, device=dev)
    graph = DeviceGraph(ei, ew, device=dev)
    del ei, ew
    sampler = RandomWalkSampler.from_graph(graph, walk_length=2, num_walks=100, rng="philox", seed=42)
    torch.manual_seed(2)
    model = PinSage(128, 256, 256, 2).to(dev).eval()
    params = {k: v.detach().float().contiguous() for k, v in model.state_dict().items()}
    x = torch.randn(M, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    return M, sampler, params, x


@pytest.mark.parametrize("T", [10, 50])
def test_layers_on_the_benchmark_batches(syn25m, T):
    """both GCN layers of the benchmark's embed pass, layer by layer, with the staged weights the pipeline uses"""
    from pinsage_hip import dense
    from pinsage_hip.shard import HipOps, fused_self_update
    M, sampler, P, x = syn25m
    ops = HipOps()
    sampler._calls = 0
    batches = list(ops.sample_layers(sampler, 0, M, T, 2))
    h = dense.linear(x, dense.stage_weight(P["input_proj.weight"]), P["input_proj.bias"], relu=True)
    H = h.size(1)
    for i, bt in enumerate(batches):
        frac = _heavy_fraction(bt.ids, bt.nvalid, M - 1)
        print(f"T={T} layer {i}: {frac:.4f} of the rows keep a neighbour")
        W1, b1 = fused_self_update(ops, P, i, H)
        Wu = P[f"convs.{i}.lin_update.weight"]
        W1s, W2s = dense.stage_weight(W1), dense.stage_weight(Wu[:, H:].contiguous())
        ref = _pair(h, W1s, b1, h, bt.ids, bt.counts, None, bt.nvalid, W2s, M - 1, 1)
        if T <= 16:
            _same(_fused(h, W1s, b1, h, bt.ids, bt.counts, None, bt.nvalid, W2s, M - 1, 1), ref)
        else:                                            # served by the pair (T > 16)
            with pytest.raises(AssertionError):
                _fused(h, W1s, b1, h, bt.ids, bt.counts, None, bt.nvalid, W2s, M - 1, 1)
        _same(dense.gcn_layer(h, W1s, b1, h, bt.ids, bt.counts, bt.nvalid, W2s, max_idx=M - 1), ref)
        h = ref


def _synthetic(T, empty, form, n_full=ROWS, max_idx=None, seed=0, zero_rows=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = torch.device("cuda")
    M, H, K = ROWS, 256, 256
    max_idx = n_full - 1 if max_idx is None else max_idx
    x = torch.randn(M, K, generator=g)
    h_full = torch.randn(n_full, H, generator=g)
    if zero_rows:                                        # rows of +0.0, of -0.0, and -0.0 entries among others
        x[:100] = 0.0
        x[100:200] = -0.0
        x[200:400, ::3] = -0.0
        h_full[:50] = -0.0
        h_full[50:300, ::2] = -0.0
    ids = torch.randint(-1, n_full + 64, (M, T), generator=g, dtype=torch.int32)       # -1 pads and ids beyond max_idx
    nvalid = torch.randint(0, T + 1, (M,), generator=g, dtype=torch.int32)
    drop = torch.rand(M, generator=g) < empty
    ids[drop] = torch.where(torch.rand((int(drop.sum()), T), generator=g) < 0.5, -1, max_idx + 1 + torch.randint(0, 9, (1,), generator=g)).to(torch.int32)
    if empty == 0.0:                                     # every row keeps entry 0
        nvalid.clamp_(min=1)
        ids[:, 0] = torch.randint(0, max_idx + 1, (M,), generator=g, dtype=torch.int32)
    counts = torch.randint(1, 40, (M, T), generator=g, dtype=torch.int32) if form == "counts" else None
    wts = torch.rand((M, T), generator=g) if form == "wts" else None
    W = torch.randn(256, K, generator=g) * 0.05
    W2 = torch.randn(256, H, generator=g) * 0.05
    b = torch.randn(256, generator=g) * 0.1
    cu = lambda t: None if t is None else t.to(dev).contiguous()
    return dict(x=cu(x), W=cu(W), b=cu(b), h_full=cu(h_full), ids=cu(ids), counts=cu(counts), wts=cu(wts), nvalid=cu(nvalid),
                W2=cu(W2), max_idx=max_idx)


@pytest.mark.parametrize("T", [1, 10, 16])
@pytest.mark.parametrize("empty", [0.0, 0.56, 1.0])
@pytest.mark.parametrize("form,renorm", [("counts", 1), ("counts", 0), ("wts", 1), ("wts", 0)])
def test_synthetic_rows(T, empty, form, renorm):
    """M not a multiple of 64; no row / about half / every row without a kept neighbour; ids above max_idx and -1 pads;
    nvalid < T; counts and weight forms; renorm 0 / 1"""
    a = _synthetic(T, empty, form, seed=T * 7 + int(empty * 100) + renorm)
    ref = _pair(**a, renorm=renorm)
    _same(_fused(**a, renorm=renorm), ref)


def test_shard_with_more_hidden_rows_than_local_rows():
    """h_full is the gathered table of all ranks (3 x the local rows); max_idx cuts it short of its end"""
    a = _synthetic(10, 0.5, "counts", n_full=3 * ROWS, max_idx=2 * ROWS + 11, seed=5)
    ref = _pair(**a, renorm=1)
    _same(_fused(**a, renorm=1), ref)


@pytest.mark.parametrize("empty", [0.0, 0.56, 1.0])
def test_zero_and_negative_zero_rows(empty):
    a = _synthetic(10, empty, "counts", seed=11, zero_rows=True)
    ref = _pair(**a, renorm=1)
    _same(_fused(**a, renorm=1), ref)


def test_staged_weights():
    from pinsage_hip import dense
    a = _synthetic(10, 0.56, "counts", seed=3)
    a["W"], a["W2"] = dense.stage_weight(a["W"]), dense.stage_weight(a["W2"])
    ref = _pair(**a, renorm=1)
    _same(_fused(**a, renorm=1), ref)


def test_unserved_shapes_and_the_switch_fall_back_to_the_pair(monkeypatch):
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    a = _synthetic(10, 0.56, "counts", seed=4)
    ref = _pair(**a, renorm=1)
    args = (a["x"], a["W"], a["b"], a["h_full"], a["ids"], a["counts"], a["nvalid"], a["W2"])
    _same(dense.gcn_layer(*args, max_idx=a["max_idx"]), ref)
    monkeypatch.setenv("PS_GCN_FUSED", "0")
    with pytest.raises(AssertionError, match=str(nv.PS_EUNSUPPORTED)):
        _fused(**a, renorm=1)
    _same(dense.gcn_layer(*args, max_idx=a["max_idx"]), ref)
    monkeypatch.delenv("PS_GCN_FUSED")
    b17 = _synthetic(17, 0.56, "counts", seed=6)                                     # T > 16
    with pytest.raises(AssertionError, match=str(nv.PS_EUNSUPPORTED)):
        _fused(**b17, renorm=1)
    _same(dense.gcn_layer(b17["x"], b17["W"], b17["b"], b17["h_full"], b17["ids"], b17["counts"], b17["nvalid"], b17["W2"],
                          max_idx=b17["max_idx"]), _pair(**b17, renorm=1))
    few = {k: (v[:1000].contiguous() if k in ("x", "ids", "counts", "nvalid") else v) for k, v in a.items()}   # below 64 x 384 rows
    with pytest.raises(AssertionError, match=str(nv.PS_EUNSUPPORTED)):
        _fused(**few, renorm=1)
    _same(dense.gcn_layer(few["x"], few["W"], few["b"], few["h_full"], few["ids"], few["counts"], few["nvalid"], few["W2"],
                          max_idx=few["max_idx"]), _pair(**few, renorm=1))


@pytest.mark.parametrize("T", [10, 50])
def test_embed_equals_the_unfused_pipeline(syn25m, T, monkeypatch):
    from pinsage_hip.shard import ShardedPinSage
    M, sampler, P, x = syn25m
    pipe = ShardedPinSage(P, 2, sampler, M)
    out = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("PS_GCN_FUSED", raising=False)
        else:
            monkeypatch.setenv("PS_GCN_FUSED", mode)
        sampler._calls = 0
        out[mode] = pipe.embed(x, T)
    _same(out[None], out["0"])
    assert np.isfinite(out[None].cpu().numpy()).all()
