"""Minibatch PinSage on the MI355X: ps_frontier_build (csrc/frontier.hip) against the numpy restatement on every case of
tests/helpers/frontier_cases.py, its error codes, and the blocks / forward built on it -- RandomWalkSampler.sample_blocks,
PinSage.forward_blocks, PinSage.embed_minibatch -- against the full-catalogue forward.

In rng="philox" mode a node's walks are keyed by (seed; node, walk, step / 2, call), so its neighbour list does not depend on the
batch it is sampled in, and the dense and pooling kernels compute a row from that row's inputs alone: the minibatch embeddings
are the full-catalogue embeddings' rows bit for bit (tests 3, 4 and 6).  One fixture holds the graph, the model, the twin
sampler's full-catalogue tables and the full forward; every test reads it and none writes it."""
import numpy as np
import pytest
import torch

from conftest import bipartite_graph
from helpers import abi_cases as ac
from helpers import abi_cases_frontier  # noqa: F401  (the entry point joins ac.CASES)
from helpers import frontier_cases as fc

pytestmark = pytest.mark.gpu
CANARY = -77
N_ITEMS, N_USERS, T, LAYERS = 2000, 500, 5, 2


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _build(seeds, ids, nvalid, T_, limit, ws_fill):
    """one direct call of the C ABI into fresh buffers -> (status, frontier buffer, count, local buffer) as numpy; every output
    is filled with CANARY and the workspace with `ws_fill` bytes beforehand"""
    from pinsage_hip import native as nv
    S, B = len(seeds), ids.shape[0]
    room = S + min(B * T_, limit)
    d_seeds, d_ids, d_nv = (_dev(a) if a.size else None for a in (seeds, ids, nvalid))
    frontier = torch.full((max(room, 1),), CANARY, dtype=torch.int32, device="cuda")
    count = torch.full((1,), CANARY, dtype=torch.int32, device="cuda")
    local = torch.full((max(B * T_, 1),), CANARY, dtype=torch.int32, device="cuda")
    nbytes = nv.lib().ps_frontier_workspace_bytes(limit, S, B, T_)
    assert nbytes > 0
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device="cuda")
    rc = nv.lib().ps_frontier_build(nv.ptr(d_seeds), S, nv.ptr(d_ids), nv.ptr(d_nv), B, T_, limit, nv.ptr(frontier), nv.ptr(count),
                                    nv.ptr(local), nv.ptr(ws), nbytes, nv.stream())
    torch.cuda.synchronize()
    return rc, frontier.cpu().numpy(), int(count.item()), local.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the kernel equals the restatement
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_kernel_equals_the_restatement(name):
    from pinsage_hip import minibatch
    seeds, ids, nvalid, T_, limit = fc.CASES[name]
    want_f, want_l = fc.restate(seeds, ids, nvalid, T_, limit)
    runs = [_build(seeds, ids, nvalid, T_, limit, fill) for fill in (0xFF, 0x5A)]      # fresh buffers, two different workspaces
    for rc, frontier, count, local in runs:
        assert rc == 0
        assert count == len(want_f) and np.array_equal(frontier[:count], want_f)
        assert np.all(frontier[count:] == CANARY)                                       # nothing written beyond count
        assert np.array_equal(local[:ids.size].reshape(ids.shape), want_l) and np.all(local[ids.size:] == CANARY)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][1::2], runs[1][1::2])) and runs[0][2] == runs[1][2]
    # the binding: device tensors in and out, None for an absent side
    got_f, got_l = minibatch.frontier(_dev(seeds) if len(seeds) else None, *((_dev(ids), _dev(nvalid)) if ids.size else (None, None)),
                                      limit)
    assert got_f.dtype == torch.int32 and got_f.is_cuda and np.array_equal(got_f.cpu().numpy(), want_f)
    if ids.size:
        assert np.array_equal(got_l.cpu().numpy(), want_l)


# ---------------------------------------------------------------------------------------------------------------- 2. error paths
def test_error_paths():
    from pinsage_hip import minibatch
    from pinsage_hip import native as nv
    lib = nv.lib()
    S, B, T_, limit = 3, 4, 2, 10
    seeds = _dev(np.array([1, 5, 9], np.int32))
    ids = _dev(np.array([[2, 5], [7, 10], [-1, 3], [2, 2]], np.int32))
    nvalid = _dev(np.array([2, 2, 2, 1], np.int32))
    frontier = torch.full((S + B * T_,), CANARY, dtype=torch.int32, device="cuda")
    count = torch.full((1,), CANARY, dtype=torch.int32, device="cuda")
    local = torch.full((B, T_), CANARY, dtype=torch.int32, device="cuda")
    nbytes = lib.ps_frontier_workspace_bytes(limit, S, B, T_)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    base = dict(seeds=seeds, S=S, ids=ids, nvalid=nvalid, B=B, T=T_, limit=limit, frontier=frontier, count=count, local=local, ws=ws,
                nbytes=nbytes)

    def call(**kw):
        a = dict(base, **kw)
        rc = lib.ps_frontier_build(nv.ptr(a["seeds"]), a["S"], nv.ptr(a["ids"]), nv.ptr(a["nvalid"]), a["B"], a["T"], a["limit"],
                                   nv.ptr(a["frontier"]), nv.ptr(a["count"]), nv.ptr(a["local"]), nv.ptr(a["ws"]), a["nbytes"], nv.stream())
        torch.cuda.synchronize()
        return rc
    # PS_EINVAL: the scalars
    for kw in (dict(T=0), dict(T=-1), dict(limit=0), dict(limit=-5), dict(limit=2 ** 31), dict(S=-1), dict(B=-1),
               dict(B=2 ** 30, T=2), dict(B=2 ** 31, T=1), dict(S=2 ** 31 - 5, limit=2 ** 31 - 1)):
        assert call(**kw) == nv.PS_EINVAL, kw
        a = dict(base, **kw)
        assert lib.ps_frontier_workspace_bytes(a["limit"], a["S"], a["B"], a["T"]) == 0, kw
    # PS_EINVAL: a null pointer on a non-empty problem
    for k in ("seeds", "ids", "nvalid", "frontier", "count", "local", "ws"):
        assert call(**{k: None}) == nv.PS_EINVAL, k
    assert call(S=0, seeds=None, ids=None) == nv.PS_EINVAL and call(B=0, ids=None, nvalid=None, local=None, seeds=None) == nv.PS_EINVAL
    # PS_EWORKSPACE
    assert call(nbytes=nbytes - 1) == nv.PS_EWORKSPACE and call(nbytes=0) == nv.PS_EWORKSPACE
    assert (frontier == CANARY).all() and (count == CANARY).all() and (local == CANARY).all()       # a refused call writes nothing
    # PS_OK for the empty problem, whatever the other pointers; count = 0 where it is given
    nothing = dict(S=0, B=0, seeds=None, ids=None, nvalid=None, frontier=None, local=None, ws=None, nbytes=0)
    assert call(**nothing) == nv.PS_OK and int(count.item()) == 0
    assert call(**dict(nothing, count=None)) == nv.PS_OK
    assert (frontier == CANARY).all() and (local == CANARY).all()
    # one side absent: B == 0 gives the seeds alone, S == 0 the sorted distinct kept ids
    count.fill_(CANARY)
    assert call(B=0, ids=None, nvalid=None, local=None) == nv.PS_OK and int(count.item()) == S
    assert frontier[:S].tolist() == [1, 5, 9] and (frontier[S:] == CANARY).all() and (local == CANARY).all()
    frontier.fill_(CANARY)
    assert call(S=0, seeds=None) == nv.PS_OK and int(count.item()) == 4
    assert frontier[:4].tolist() == [2, 3, 5, 7] and (frontier[4:] == CANARY).all()
    assert local.tolist() == [[0, 2], [3, -1], [-1, 1], [0, -1]]
    # and the whole problem
    frontier.fill_(CANARY)
    assert call() == nv.PS_OK and int(count.item()) == 6 and frontier[:6].tolist() == [1, 5, 9, 2, 3, 7]
    assert local.tolist() == [[3, 1], [5, -1], [-1, 4], [3, -1]] and (frontier[6:] == CANARY).all()
    # the binding names what it refuses
    with pytest.raises(TypeError):
        minibatch.frontier(seeds.long(), ids, nvalid, limit)
    with pytest.raises(TypeError):
        minibatch.frontier(seeds, ids, nvalid.cpu(), limit)
    with pytest.raises(ValueError):
        minibatch.frontier(seeds, ids, None, limit)
    with pytest.raises(ValueError):
        minibatch.frontier(None, None, None, limit)
    with pytest.raises(ValueError):
        minibatch.frontier(seeds, ids, nvalid, 0)
    with pytest.raises(ValueError):
        minibatch.frontier(seeds, ids, nvalid, 2 ** 31)


def test_seeds_outside_the_contract_stay_inside_the_buffers():
    """a seed beyond [0, limit) or listed twice: the outputs are unspecified, the guard entries behind the buffers are not"""
    seeds = np.array([4, 300, -2, 4, 2 ** 31 - 1, 7], np.int32)
    ids = np.array([[4, 7, 1], [300, 2, 4]], np.int32)
    rc, frontier, count, local = _build(seeds, ids, np.array([3, 3], np.int32), 3, 10, 0xFF)
    assert rc == 0 and 0 <= count <= len(seeds) + 6
    assert np.array_equal(frontier[:len(seeds)], seeds)                                 # copied, never used as an index
    assert np.all((local >= -1) & (local < len(seeds) + 6))


def test_contract_matrix_holds_the_frontier():
    """The contract matrix of tests/test_hip_abi_contract.py (captured stream, poisoned outputs and workspace, guard bands, replays)
    for the entry point, started from here as well: that module parametrises over the case table when it is collected, and a run
    of it alone does not import the case module of this entry point."""
    import test_hip_abi_contract as contract
    assert "ps_frontier_build" in ac.CASES
    contract.test_contract("ps_frontier_build")


# ---------------------------------------------------------------------------------------------------------------- the shared fixture
def _sampler(world, **kw):
    from utils.random_walk import RandomWalkSampler
    args = dict(walk_length=2, num_walks=20, rng="philox", seed=1234)
    args.update(kw)
    return RandomWalkSampler.from_graph(world["graph"], **args)


def _host_tables(batches):
    return [(b.ids.cpu().numpy(), b.nvalid.cpu().numpy(), b.counts.cpu().numpy()) for b in batches]


def _lists(batches):
    from pinsage_hip import sampling
    return ([sampling.LazyNeighborList(b, "ids") for b in batches], [sampling.LazyNeighborList(b, "weights") for b in batches])


def _same_blocks(blocks, want, payload="counts"):
    for i, (b, w) in enumerate(zip(blocks, want)):
        assert b.n_dst == w["n_dst"] and np.array_equal(b.src_nodes.cpu().numpy(), w["src_nodes"]), f"block {i}: nodes"
        assert np.array_equal(b.ids.cpu().numpy(), w["ids"]), f"block {i}: ids"
        assert np.array_equal(b.nvalid.cpu().numpy(), w["nvalid"]), f"block {i}: nvalid"
        assert np.array_equal(getattr(b, payload).cpu().numpy(), w["payload"]), f"block {i}: {payload}"
    assert len(blocks) == len(want)


@pytest.fixture(scope="module")
def world():
    from model.pinsage import PinSage
    from utils.random_walk import RandomWalkSampler
    dev = torch.device("cuda:0")
    ei, ew = bipartite_graph(N_ITEMS, N_USERS, 12000, seed=11)
    first = RandomWalkSampler(torch.from_numpy(ei), torch.from_numpy(ew), walk_length=2, num_walks=20, device=dev, rng="philox", seed=1234)
    w = dict(graph=first.graph, dev=dev)
    torch.manual_seed(5)
    w["model"] = PinSage(24, 32, 16, LAYERS).to(dev)
    w["x"] = torch.randn(N_ITEMS, 24, device=dev)
    seeds = np.random.RandomState(3).randint(0, N_ITEMS, 29)
    seeds[28] = seeds[0]                                                                 # one repeated
    w["seeds"] = seeds
    # the twin: the full-catalogue tables of calls 0 and 1, and the full forward over them
    twin = RandomWalkSampler(torch.from_numpy(ei), torch.from_numpy(ew), walk_length=2, num_walks=20, device=dev, rng="philox", seed=1234)
    w["full_batches"] = twin.sample_batches(range(N_ITEMS), T, LAYERS)
    w["tables"] = _host_tables(w["full_batches"])
    nb, wt = _lists(w["full_batches"])
    with torch.no_grad():
        w["full"] = w["model"](w["x"], sampled_neighbors=nb, importance_weights=wt)
    # the blocks, from the first sampler (calls 0 and 1 as well)
    w["input_nodes"], w["inverse"], w["blocks"] = first.sample_blocks(seeds, T, LAYERS, n_items=N_ITEMS)
    assert first._calls == LAYERS == twin._calls
    w["want"] = fc.restate_blocks(seeds, w["tables"], N_ITEMS)
    torch.cuda.synchronize()
    return w


# ------------------------------------------------------------------------------------- 3. minibatch equals catalogue, without gradients
def test_minibatch_equals_catalogue(world):
    w = world
    seeds, blocks = w["seeds"], w["blocks"]
    want_in, want_inv, want = w["want"]
    # the fixture is the one the bit-equality is worth checking on
    assert len(seeds) == 29 and len(set(seeds.tolist())) == 28
    assert [b.n_dst for b in blocks] == [48, 28] and [b.n_src for b in blocks] == [89, 48]
    top_ids = blocks[1].ids.cpu().numpy()
    raw_top = w["tables"][1][0][np.unique(seeds)]
    assert raw_top.size == 140 and int((raw_top >= N_ITEMS).sum()) == 116
    for i, b in enumerate(blocks):
        assert b.n_dst < b.n_src < N_ITEMS                                               # grows at every layer, below the catalogue
        loc = b.ids.cpu().numpy()
        raw = w["tables"][i][0][b.src_nodes[:b.n_dst].cpu().numpy()]
        assert (loc >= 0).any() and ((loc < 0) & (raw >= N_ITEMS)).any()                 # kept slots and dropped user slots
        rows = np.nonzero(loc >= 0)[0]
        readers = {r: {r} for r in range(b.n_dst)}                                       # row r reads source row r as itself
        for r, p in zip(rows, loc[loc >= 0]):
            readers.setdefault(int(p), set()).add(int(r))
        assert any(len(rs) > 1 for rs in readers.values())                               # a source row read by two rows
    assert top_ids.shape == (28, T)
    # the blocks are the restatement applied to the twin's full tables
    _same_blocks(blocks, want)
    assert np.array_equal(w["input_nodes"].cpu().numpy(), want_in) and np.array_equal(w["inverse"].cpu().numpy(), want_inv)
    assert w["input_nodes"].dtype == torch.int32 and w["inverse"].dtype == torch.int64
    # and the embeddings are the catalogue's rows, bit for bit
    model, x = w["model"], w["x"]
    seeds_t = torch.from_numpy(seeds).to(w["dev"])
    with torch.no_grad():
        mini = model.embed_minibatch(x, _sampler(w), seeds, T)
        again = model.forward_blocks(x[w["input_nodes"].long()], blocks)[w["inverse"]]
    assert mini.shape == (29, 16) and torch.equal(mini, w["full"][seeds_t])
    assert torch.equal(again, mini)
    assert float(mini.abs().max()) > 0 and not torch.equal(mini[0], mini[1])


# --------------------------------------------------------------------------------------------------------------- 4. the same, on the tape
def _forward64(P, x_in, blocks):
    """the block forward in float64 torch on the CPU (exact weights count / sum of the kept counts), differentiable"""
    F = torch.nn.functional
    h = torch.relu(x_in @ P["input_proj.weight"].t() + P["input_proj.bias"])
    for i, b in enumerate(blocks):
        ids, nvalid, counts = (t.cpu() for t in (b.ids, b.nvalid, b.counts))
        keep = (torch.arange(ids.size(1))[None, :] < nvalid.clamp(0, ids.size(1))[:, None]) & (ids >= 0)
        wgt = torch.where(keep, counts.double(), torch.zeros((), dtype=torch.float64))
        tot = wgt.sum(1, keepdim=True)
        wgt = torch.where(tot > 0, wgt / torch.where(tot > 0, tot, torch.ones_like(tot)), wgt)
        h_neigh = (h[torch.where(keep, ids, torch.zeros_like(ids)).long()] * wgt[:, :, None]).sum(1)
        h_self = h[:b.n_dst] @ P[f"convs.{i}.lin_self.weight"].t() + P[f"convs.{i}.lin_self.bias"]
        h = torch.relu(torch.cat([h_self, h_neigh], 1) @ P[f"convs.{i}.lin_update.weight"].t() + P[f"convs.{i}.lin_update.bias"])
        h = F.normalize(h, p=2, dim=1)
    return F.normalize(h @ P["output_proj.weight"].t() + P["output_proj.bias"], p=2, dim=1)


def _grads(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    return {k: p.grad.detach().double().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


def _square_sum(out):
    return out.square().sum()


def _weighted_sum(out):
    """sum(out * C) with a fixed cotangent C: the rows of `out` are unit vectors, so sum(out^2) is the constant len(out) and its
    true gradient is zero; this loss has one that is not"""
    C = torch.from_numpy(np.random.RandomState(12).standard_normal(tuple(out.shape))).to(device=out.device, dtype=out.dtype)
    return (out * C).sum()


@pytest.mark.parametrize("loss", [_square_sum, _weighted_sum], ids=["square_sum", "weighted_sum"])
def test_minibatch_equals_catalogue_on_the_tape(world, monkeypatch, loss):
    """Forward: the rows of the full tape forward, bit for bit.  Gradients: per parameter tensor the max-norm error of the HIP
    gradients against a float64 restatement may be at most 4 x the error of the fp32 grad_method = "torch" path against the same
    float64 values (an allowance for a different summation order, not a measured figure); the full-catalogue HIP gradients are held
    to the same bound, so the two HIP gradients may differ by at most 8 x it.
    square_sum is sum(mini^2): the embeddings are unit rows, so its true gradient is zero (1e-15 in float64) and all three fp32
    gradients are rounding noise of 1e-7 around it.  weighted_sum has gradients of order 1.

    Observed on the MI355X (run with -s for the table), err(HIP) / err(torch) over the twelve parameter tensors:
      square_sum    minibatch 0.48 .. 1.23 (largest: output_proj.weight), full catalogue the same figures; the two HIP gradients
                    differ by at most 1.1e-13 where the torch path's error is 5.8e-08 .. 8.0e-07
      weighted_sum  minibatch 0.65 .. 1.68 (largest: output_proj.bias), full catalogue 0.77 .. 2.20 (output_proj.bias); the two
                    HIP gradients differ by at most 2.4e-06 (output_proj.bias, |g| = 27) where the torch path's error is
                    3.7e-07 .. 8.1e-06"""
    from pinsage_hip import sampling
    w = world
    model, x, blocks, inverse = w["model"], w["x"], w["blocks"], w["inverse"]
    seeds_t = torch.from_numpy(w["seeds"]).to(w["dev"])
    x_in = x[w["input_nodes"].long()]
    nb, wt = _lists(w["full_batches"])
    monkeypatch.setattr(sampling, "grad_method", "hip")
    assert all(p.requires_grad for p in model.parameters()) and torch.is_grad_enabled()
    full = model(x, sampled_neighbors=nb, importance_weights=wt)
    mini = model.forward_blocks(x_in, blocks)[inverse]
    assert mini.requires_grad and torch.equal(mini, full[seeds_t])
    g_mini = _grads(model, loss(mini))
    g_full = _grads(model, loss(full[seeds_t]))
    monkeypatch.setattr(sampling, "grad_method", "torch")
    g_torch = _grads(model, loss(model.forward_blocks(x_in, blocks)[inverse]))
    monkeypatch.setattr(sampling, "grad_method", "hip")
    # float64 on the CPU
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters()}
    out64 = _forward64(P, x_in.double().cpu(), blocks)[inverse.cpu()]
    assert float((out64.detach() - mini.detach().double().cpu()).abs().max()) < 1e-5
    loss(out64).backward()
    g64 = {k: v.grad for k, v in P.items() if v.grad is not None}
    used = sorted(k for k in g64 if float(g64[k].abs().max()) > 0)
    assert set(used) == set(g_mini) == set(g_full) == set(g_torch) and len(used) == 12    # every layer but the unused lin_neigh
    rows = []
    for k in used:
        e_torch = float((g_torch[k] - g64[k]).abs().max())
        e_mini = float((g_mini[k] - g64[k]).abs().max())
        e_full = float((g_full[k] - g64[k]).abs().max())
        d = float((g_mini[k] - g_full[k]).abs().max())
        print(f"{k:28s} |g| {float(g64[k].abs().max()):.3e}  torch {e_torch:.3e}  hip mini {e_mini:.3e} ({e_mini / e_torch:.2f} x)  "
              f"hip full {e_full:.3e} ({e_full / e_torch:.2f} x)  mini - full {d:.3e}")
        rows.append((k, e_torch, e_mini, e_full, d))
    for k, e_torch, e_mini, e_full, d in rows:
        assert e_torch > 0, k
        assert e_mini <= 4 * e_torch, f"{k}: HIP minibatch gradient {e_mini:.3e} from float64, torch {e_torch:.3e}"
        assert e_full <= 4 * e_torch, f"{k}: HIP full-catalogue gradient {e_full:.3e} from float64, torch {e_torch:.3e}"
        assert d <= 8 * e_torch, f"{k}: minibatch and full-catalogue gradients differ by {d:.3e}, torch error {e_torch:.3e}"


# -------------------------------------------------------------------------------------------------------------------- 5. rng = "numpy"
def test_numpy_stream_blocks(world):
    w = world
    seeds = w["seeds"]
    a, b = _sampler(w, rng="numpy"), _sampler(w, rng="numpy")
    np.random.seed(7)
    input_nodes, inverse, blocks = a.sample_blocks(seeds, T, LAYERS, n_items=N_ITEMS)
    state_a = np.random.get_state()
    # by hand: the top layer for the distinct seeds, then the layer below for that block's sources, one sample_batch each
    np.random.seed(7)
    nodes, want_inv = np.unique(seeds, return_inverse=True)
    nodes = nodes.astype(np.int32)
    want = [None] * LAYERS
    for i in (1, 0):
        batch = b.sample_batch(nodes.astype(np.int64), T)
        ids, nvalid, counts = batch.ids.cpu().numpy(), batch.nvalid.cpu().numpy(), batch.counts.cpu().numpy()
        src, local = fc.restate(nodes, ids, nvalid, T, N_ITEMS)
        want[i] = dict(src_nodes=src, n_dst=len(nodes), ids=local, nvalid=nvalid, payload=counts)
        nodes = src
    state_b = np.random.get_state()
    _same_blocks(blocks, want)
    assert np.array_equal(input_nodes.cpu().numpy(), want[0]["src_nodes"]) and np.array_equal(inverse.cpu().numpy(), want_inv.reshape(-1))
    assert state_a[0] == state_b[0] and np.array_equal(state_a[1], state_b[1]) and state_a[2:] == state_b[2:]
    assert np.random.random_sample() != np.random.RandomState(7).random_sample()          # the stream has moved
    assert a._calls == b._calls == LAYERS
    assert blocks[0].n_src > blocks[0].n_dst > blocks[1].n_dst


# -------------------------------------------------------------------------------------------------------------------- 6. source = "ppr"
def test_ppr_blocks(world):
    w = world
    model, x, seeds = w["model"], w["x"], w["seeds"]
    sampler = _sampler(w)
    wb = sampler.ppr_batch(range(N_ITEMS), T, max_target=N_ITEMS)
    seeds_t = torch.from_numpy(seeds).to(w["dev"])
    with torch.no_grad():
        full = model(x, sampled_neighbors=[wb] * LAYERS, importance_weights=[wb] * LAYERS)
        mini = model.embed_minibatch(x, sampler, seeds, T, source="ppr")
    assert torch.equal(mini, full[seeds_t]) and not torch.equal(full, w["full"])
    assert sampler._calls == 0                                                          # no RNG, no call numbers
    table = (wb.ids.cpu().numpy(), wb.nvalid.cpu().numpy(), wb.wts.cpu().numpy())
    _, _, blocks = sampler.sample_blocks(seeds, T, LAYERS, n_items=N_ITEMS, source="ppr")
    _same_blocks(blocks, fc.restate_blocks(seeds, [table] * LAYERS, N_ITEMS)[2], payload="wts")
    assert all(b.counts is None and b.wts.dtype == torch.float64 for b in blocks) and blocks[0].n_src > blocks[1].n_src > 28


# -------------------------------------------------------------------------------------------------------------------- 7. biased walks
def test_biased_walk_blocks(world):
    w = world
    a, b = _sampler(w, p=0.5, q=2.0), _sampler(w, p=0.5, q=2.0)
    input_nodes, inverse, blocks = a.sample_blocks(w["seeds"], T, LAYERS, n_items=N_ITEMS)
    tables = _host_tables(b.sample_batches(range(N_ITEMS), T, LAYERS))
    want_in, want_inv, want = fc.restate_blocks(w["seeds"], tables, N_ITEMS)
    _same_blocks(blocks, want)
    assert np.array_equal(input_nodes.cpu().numpy(), want_in) and np.array_equal(inverse.cpu().numpy(), want_inv)
    assert any(not np.array_equal(t[0], u[0]) for t, u in zip(tables, w["tables"]))      # not the first-order walk's lists


# -------------------------------------------------------------------------------------------------------------------- 8. a user-node seed
def test_a_seed_outside_the_items_is_refused(world):
    w = world
    sampler = _sampler(w)
    for bad in ([3, N_ITEMS], [N_ITEMS + N_USERS - 1], [-1, 4], torch.tensor([5, N_ITEMS], device=w["dev"])):
        with pytest.raises(ValueError):
            sampler.sample_blocks(bad, T, LAYERS, n_items=N_ITEMS)
        with pytest.raises(ValueError):
            w["model"].embed_minibatch(w["x"], sampler, bad, T)
    assert sampler._calls == 0                                                          # a refused request reserves nothing
    with pytest.raises(ValueError):
        sampler.sample_blocks([3], T, LAYERS, n_items=N_ITEMS, source="edges")
    with pytest.raises(ValueError):
        w["model"].forward_blocks(w["x"][:89], w["blocks"][:1])
    # without n_items every node of the graph may be a seed, and user ids stay in the blocks
    _, _, blocks = sampler.sample_blocks([3, N_ITEMS], T, 1)
    assert int(blocks[0].src_nodes.max()) >= N_ITEMS
