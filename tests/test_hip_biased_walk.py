"""Node2vec-biased walks on the device (csrc/walk_biased.hip: ps_walk_paths_biased; csrc/walk_topk.hip: ps_paths_topk) and the
p / q of RandomWalkSampler, against tests/helpers/biased_walk_cases.py -- the reference's loop with the alpha multiplication, drawing from
np.random.  Every comparison is exact.

  1. bias {1, 1} is ps_walk_paths bit for bit (stream and Philox, walk_mod 0 and W, L 1 .. 5);
  2. ps_paths_topk over replayed paths is ps_walk_sample's ids / counts / nvalid (both run csrc/walk_visits.h: the callers' glue),
     and equals the restatement at every number of positions per lane and every padding edge;
  3. rng='numpy': the sampler's paths, neighbour lists, fp64 weights and np.random state equal the restatement's;
  4. planted uniforms (ties on the biased CDF, 0, 1 - 2^-53) land where np.searchsorted puts them, on a row of every degree;
  5. the surface: argument errors, graphs with sinks, from_graph, hard negatives, the sharded pipeline's refusal, the untouched
     default path;
  6. the C ABI's contract for the two entry points (the capture / stream / guard-band matrix is tests/test_hip_abi_contract.py,
     which reads their cases from tests/helpers/abi_cases_biased.py).
A bias entry that is not finite and positive cannot be answered with PS_EINVAL: `bias` is device memory and no entry point
synchronises (include/pinsage_hip.h).  The kernel answers it -- every path of the call is -1 -- and the Python layer raises
ValueError before anything is launched; both are checked here."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import biased_walk_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def graphs():
    """{sinks: (DeviceGraph, adj_list, out_sets, info, V)} of the case graph"""
    from pinsage_hip.graph import DeviceGraph
    out = {}
    for sinks in (False, True):
        ei, w, V, info, adj, outs = bc.case_graph(sinks)
        g = DeviceGraph(torch.from_numpy(ei), torch.from_numpy(w))
        assert g.V == V and g.has_reachable_sink == sinks
        out[sinks] = (g, adj, outs, info, V)
    return out


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _biased_abi(g, starts, L, mode, uniforms, uoff, seed, call, walk_mod, bias):
    from pinsage_hip import native as nv
    paths = torch.full((starts.numel(), L), -7, dtype=torch.int32, device="cuda")
    nv.call("ps_walk_paths_biased", nv.ptr(g.rowptr), nv.ptr(g.col), nv.ptr(g.wsorted), nv.ptr(g.cdf), nv.ptr(g.sorted_neighbors()),
            g.V, nv.ptr(starts), starts.numel(), L, mode, nv.ptr(uniforms), nv.ptr(uoff), seed, call, walk_mod, nv.ptr(bias),
            nv.ptr(paths), nv.stream())
    return paths


def _plain_abi(g, starts, L, mode, uniforms, uoff, seed, call, walk_mod):
    from pinsage_hip import native as nv
    paths = torch.full((starts.numel(), L), -7, dtype=torch.int32, device="cuda")
    nv.call("ps_walk_paths", nv.ptr(g.rowptr), nv.ptr(g.col), nv.ptr(g.cdf), g.V, nv.ptr(starts), starts.numel(), L, mode,
            nv.ptr(uniforms), nv.ptr(uoff), seed, call, walk_mod, nv.ptr(g.nodeinfo), nv.ptr(g.guide), nv.ptr(paths), nv.stream())
    return paths


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ------------------------------------------------------------------------------------------------------------ 1. identity

@pytest.mark.parametrize("L", [1, 2, 3, 5])
def test_unit_bias_is_the_plain_walk(graphs, L):
    from pinsage_hip import native as nv
    g, _, _, _, V = graphs[False]
    W = 4
    starts = _dev(np.repeat(np.arange(V), W), np.int64)
    B = starts.numel()
    one = _dev([1.0, 1.0])
    rs = np.random.RandomState(10 + L)
    u = _dev(rs.random_sample(B * L))
    uoff = _dev(rs.permutation(B) * L, np.int64)
    a = _biased_abi(g, starts, L, nv.PS_RNG_STREAM, u, uoff, 0, 0, 0, one)
    b = _plain_abi(g, starts, L, nv.PS_RNG_STREAM, u, uoff, 0, 0, 0)
    assert torch.equal(a, b) and bool((a >= 0).all())
    for walk_mod in (0, W):
        a = _biased_abi(g, starts, L, nv.PS_RNG_PHILOX, None, None, 0x1234567890, 3, walk_mod, one)
        b = _plain_abi(g, starts, L, nv.PS_RNG_PHILOX, None, None, 0x1234567890, 3, walk_mod)
        assert torch.equal(a, b) and bool((a >= 0).all())
    # and on the graph with sinks (Philox): the same -1 tails
    gs = graphs[True][0]
    a = _biased_abi(gs, starts, L, nv.PS_RNG_PHILOX, None, None, 5, 1, W, one)
    b = _plain_abi(gs, starts, L, nv.PS_RNG_PHILOX, None, None, 5, 1, W)
    assert torch.equal(a, b) and bool((a < 0).any())


# ------------------------------------------------------------------------------------------------------------ 2. counting

@pytest.mark.parametrize("W,L,T", [(100, 2, 10), (100, 2, 200), (7, 3, 50), (1, 1, 1)])
def test_paths_topk_is_the_samplers_counting(graphs, W, L, T):
    from pinsage_hip import native as nv
    from pinsage_hip import sampling
    g, _, _, info, V = graphs[True]
    nodes = np.concatenate([np.arange(0, V, 3), info["sink"][:3]])         # starts without out-edges among them
    want = sampling.walk_sample(g, nodes, T, W=W, L=L, rng="philox", seed=99, call=7)
    starts = _dev(np.repeat(nodes, W), np.int64)
    paths = _plain_abi(g, starts, L, nv.PS_RNG_PHILOX, None, None, 99, 7, W)
    got = sampling.paths_topk(paths.view(len(nodes), W * L), T)
    assert torch.equal(got.ids, want.ids) and torch.equal(got.counts, want.counts) and torch.equal(got.nvalid, want.nvalid)
    assert int(want.nvalid[-1]) == 0 and int(want.nvalid.max()) > 0
    # the restatement agrees (Counter insertion order under a stable sort)
    ids, counts, nvalid = bc.topk_from_paths(paths.view(len(nodes), W * L).cpu().numpy(), T)
    assert np.array_equal(ids, got.ids.cpu().numpy()) and np.array_equal(counts, got.counts.cpu().numpy())
    assert np.array_equal(nvalid, got.nvalid.cpu().numpy())


def test_paths_topk_on_hand_written_paths():
    from pinsage_hip import sampling
    paths = np.array([[5, -1, 9, 5, -1, 2, 9, 5],        # counts 3, 2, 1
                      [4, 3, 2, 1, 8, 7, 6, 5],          # all equal: first-visit order
                      [-1, -1, 3, -1, 1, -1, 3, 1],      # a tie between 3 and 1: 3 was seen first
                      [-1] * 8,
                      [6] * 8], dtype=np.int32)
    for T in (1, 3, 8, 11):
        got = sampling.paths_topk(_dev(paths), T)
        ids, counts, nvalid = bc.topk_from_paths(paths, T)
        assert np.array_equal(got.ids.cpu().numpy(), ids) and np.array_equal(got.counts.cpu().numpy(), counts)
        assert np.array_equal(got.nvalid.cpu().numpy(), nvalid)
    assert ids[0, :3].tolist() == [5, 9, 2] and ids[1, :8].tolist() == [4, 3, 2, 1, 8, 7, 6, 5] and ids[2, :2].tolist() == [3, 1]
    assert nvalid.tolist() == [3, 8, 2, 0, 1]


def _register_rows(n):
    """five rows of n entries: many classes with ties and -1 holes; all distinct; all equal; all -1; one id at the even positions
    among distinct ones (count ceil(n / 2) against ones)"""
    rs = np.random.RandomState(1000 + n)
    mixed = rs.randint(0, max(2, n // 3), size=n)
    mixed[rs.random_sample(n) < 0.1] = -1
    alternating = 100000 + np.arange(n)
    alternating[::2] = 7
    return np.stack([mixed, 10 + rs.permutation(8 * n)[:n], np.full(n, 42), np.full(n, -1), alternating]).astype(np.int32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2049, 4095])
def test_paths_topk_on_register_positions(n):
    """ps_paths_topk keeps a row's positions in registers, NP = 1, 2, 4 .. 64 per lane (csrc/walk_topk.hip): n on either side of
    every NP's last lane group and of the 33-word bitmap, n that is no multiple of 64, T below, inside and at n."""
    from pinsage_hip import sampling
    paths = _register_rows(n)
    if n >= 8:                                                    # the first row has a tie between different ids
        c = np.bincount(paths[0][paths[0] >= 0])
        c = c[c > 0]
        assert np.unique(c).size < c.size
    dev = _dev(paths)
    for T in sorted({1, 7, n}):
        ids, counts, nvalid = bc.topk_from_paths(paths, T)
        assert nvalid[3] == 0 and nvalid[2] == 1 and (ids[4, 0], counts[4, 0]) == (7, (n + 1) // 2)
        got = sampling.paths_topk(dev, T)
        assert np.array_equal(got.ids.cpu().numpy(), ids), T
        assert np.array_equal(got.counts.cpu().numpy(), counts), T
        assert np.array_equal(got.nvalid.cpu().numpy(), nvalid), T


# ------------------------------------------------------------------------------------------- 3. rng='numpy' vs the restatement

def _case_nodes(info):
    r, t = info["returner"]
    a, _ = info["parallel"]
    return [v[0] for v in info["class"].values()] + [t, r, info["self_loop"], a, info["nclass"] + 9]


@pytest.mark.parametrize("p,q", bc.BIASES)
@pytest.mark.parametrize("L", [2, 3])
def test_numpy_stream_equals_the_restatement(graphs, p, q, L):
    from utils.random_walk import RandomWalkSampler
    g, adj, outs, info, V = graphs[False]
    W, T = 12, 10
    s = RandomWalkSampler.from_graph(g, walk_length=L, num_walks=W, p=p, q=q)
    inv_p, inv_q = 1.0 / p, 1.0 / q
    nodes = _case_nodes(info)
    # single_walks / _single_walk
    starts = nodes * 3
    np.random.seed(500 + L)
    want = [bc.single_walk(adj, v, L, inv_p, inv_q, outs) for v in starts]
    state = np.random.get_state()
    np.random.seed(500 + L)
    got = s.single_walks(starts).cpu().numpy()
    assert _state_equal(np.random.get_state(), state)
    assert got.tolist() == [w[1:] for w in want]
    np.random.seed(600 + L)
    want = bc.single_walk(adj, nodes[5], L, inv_p, inv_q, outs)
    state = np.random.get_state()
    np.random.seed(600 + L)
    got = s._single_walk(nodes[5])
    assert got == want and _state_equal(np.random.get_state(), state)
    # batch_sample_neighbors: ids, fp64 weights, stream state
    np.random.seed(700 + L)
    want = [bc.sample_neighbors(adj, v, T, W, L, inv_p, inv_q, outs) for v in nodes]
    state = np.random.get_state()
    np.random.seed(700 + L)
    nb, wt = s.batch_sample_neighbors(nodes, T)
    assert _state_equal(np.random.get_state(), state)
    assert [list(map(int, x)) for x in nb] == [list(map(int, x[0])) for x in want]
    assert [list(x) for x in wt] == [x[1] for x in want]
    np.random.seed(800 + L)
    w1 = bc.sample_neighbors(adj, nodes[3], T, W, L, inv_p, inv_q, outs)
    np.random.seed(800 + L)
    one = s.sample_neighbors(nodes[3], T)
    assert list(map(int, one[0])) == list(map(int, w1[0])) and one[1] == w1[1]
    # sample_batches(layers=2) = two consecutive calls
    np.random.seed(900 + L)
    both = s.sample_batches(nodes, T, layers=2)
    state = np.random.get_state()
    np.random.seed(900 + L)
    first, second = s.sample_batch(nodes, T), s.sample_batch(nodes, T)
    assert _state_equal(np.random.get_state(), state)
    for a, b in zip(both, (first, second)):
        assert torch.equal(a.ids, b.ids) and torch.equal(a.counts, b.counts) and torch.equal(a.nvalid, b.nvalid)
    assert not torch.equal(first.ids, second.ids)


def test_the_bias_steers_the_walk(graphs):
    """The share of two-step walks that return to their start, under Philox, against its exact expectation from the restatement's
    probabilities: sum over the edges s -> v of P(v | s) * P(s | v, came from s).  N independent walks return with a binomial
    count; the bound is five standard deviations of it.  p = 0.25 returns more often than p = 4."""
    from utils.random_walk import RandomWalkSampler
    g, adj, outs, _, V = graphs[False]
    R = 100
    starts = np.repeat(np.arange(V), R)
    share = {}
    for p in (0.25, 4.0):
        expect = 0.0
        for s0 in range(V):
            dest, w = bc.biased_weights(adj, outs, s0, None, 1.0, 1.0)
            first = w / w.sum()
            for v in set(dest):
                if s0 in outs[v]:
                    d2, w2 = bc.biased_weights(adj, outs, v, s0, 1.0 / p, 1.0)
                    expect += first[np.array(dest) == v].sum() * w2[np.array(d2) == s0].sum() / w2.sum()
        expect /= V
        s = RandomWalkSampler.from_graph(g, walk_length=2, num_walks=1, rng="philox", seed=3, p=p, q=1.0)
        paths = s.single_walks(starts).cpu().numpy()
        share[p] = float((paths[:, 1] == starts).mean())
        sigma = np.sqrt(expect * (1.0 - expect) / starts.size)
        print(f"p={p}: {share[p]:.5f} of {starts.size} walks return, expected {expect:.5f}, sigma {sigma:.5f}")
        assert abs(share[p] - expect) < 5.0 * sigma
    assert share[0.25] > share[4.0]


# ------------------------------------------------------------------------------------------------------ 4. planted uniforms

@pytest.mark.parametrize("p,q", [(0.25, 4.0), (4.0, 0.25)])
def test_planted_uniforms_land_on_searchsorted(graphs, p, q):
    from pinsage_hip import native as nv
    from pinsage_hip import sampling
    g, _, _, _, V = graphs[False]
    pl = bc.planted_paths(p, q)
    L = bc.PLANT_L
    B = pl.starts.size
    u = _dev(pl.uniforms)
    got = _biased_abi(g, _dev(pl.starts), L, nv.PS_RNG_STREAM, u, _dev(np.arange(B) * L, np.int64), 0, 0, 0, _dev([1.0 / p, 1.0 / q]))
    got = got.cpu().numpy()
    bad = np.argwhere(got != pl.picks)
    assert bad.size == 0, [(int(i), int(st), bc.KINDS[pl.kind[i, st]], int(pl.deg[i, st]), int(got[i, st]), int(pl.picks[i, st]))
                           for i, st in bad[:8]]
    # through the sampler's `uniforms=`: one walk per start node, the visit histogram of the planted path
    batch = sampling.walk_sample(g, pl.starts, L, W=1, L=L, rng="numpy", uniforms=u, p=p, q=q)
    ids, counts, nvalid = bc.topk_from_paths(pl.picks, L)
    assert np.array_equal(batch.ids.cpu().numpy(), ids) and np.array_equal(batch.counts.cpu().numpy(), counts)
    assert np.array_equal(batch.nvalid.cpu().numpy(), nvalid)


# ------------------------------------------------------------------------------------------------------------- 4b. long rows
# The kernel treats a row by its length (csrc/walk_biased.hip): products kept in LDS up to 1024 edges and recomputed beyond, a
# second buffer of numpy's sum beyond 8192, the chain replayed past the 128 kept accumulators beyond 8192.  The long-row graph has
# a row on either side of each (tests/test_biased_walk_cases.py proves what the planted batch reaches).

@pytest.fixture(scope="module")
def long_graph():
    from pinsage_hip.graph import DeviceGraph
    ei, w, V, info, adj, outs = bc.long_graph()
    g = DeviceGraph(torch.from_numpy(ei), torch.from_numpy(w))
    assert g.V == V and not g.has_reachable_sink and g.max_degree == max(bc.LONG_DEGREES)
    return g, adj, outs, info, V


@pytest.mark.parametrize("p,q", [(0.25, 4.0), (4.0, 0.25)])
def test_planted_uniforms_on_long_rows(long_graph, p, q):
    from pinsage_hip import native as nv
    g = long_graph[0]
    pl = bc.planted_long_paths(p, q)
    L, B = bc.LONG_L, pl.starts.size
    got = _biased_abi(g, _dev(pl.starts), L, nv.PS_RNG_STREAM, _dev(pl.uniforms), _dev(np.arange(B) * L, np.int64), 0, 0, 0,
                      _dev([1.0 / p, 1.0 / q])).cpu().numpy()
    bad = np.argwhere(got != pl.picks)
    assert bad.size == 0, [(int(i), int(st), bc.KINDS[pl.kind[i, st]], int(pl.deg[i, st]), int(pl.target[i, st]), int(got[i, st]),
                            int(pl.picks[i, st])) for i, st in bad[:8]]


@pytest.mark.parametrize("L", [2, 3])
def test_unit_bias_is_the_plain_walk_on_long_rows(long_graph, L):
    from pinsage_hip import native as nv
    g, _, _, _, V = long_graph
    W = 64
    starts = _dev(np.repeat(np.arange(V), W), np.int64)
    B = starts.numel()
    one = _dev([1.0, 1.0])
    rs = np.random.RandomState(20 + L)
    u = rs.random_sample(B * L)
    u[::7], u[3::11] = 0.0, bc.U_MAX                                  # the first and the last edge of whatever row
    u, uoff = _dev(u), _dev(np.arange(B) * L, np.int64)
    a = _biased_abi(g, starts, L, nv.PS_RNG_STREAM, u, uoff, 0, 0, 0, one)
    b = _plain_abi(g, starts, L, nv.PS_RNG_STREAM, u, uoff, 0, 0, 0)
    assert torch.equal(a, b) and bool((a >= 0).all())
    # every hub was stood on after the first step
    stood = torch.unique(a[:, :-1]).tolist()
    assert set(range(len(bc.LONG_DEGREES))) <= set(stood)
    a = _biased_abi(g, starts, L, nv.PS_RNG_PHILOX, None, None, 77, 2, W, one)
    b = _plain_abi(g, starts, L, nv.PS_RNG_PHILOX, None, None, 77, 2, W)
    assert torch.equal(a, b)


def test_numpy_stream_on_long_rows(long_graph):
    from utils.random_walk import RandomWalkSampler
    g, adj, outs, info, V = long_graph
    p, q, L = 0.25, 4.0, 3
    s = RandomWalkSampler.from_graph(g, walk_length=L, num_walks=5, p=p, q=q)
    starts = list(range(V)) * 2
    np.random.seed(321)
    want = [bc.single_walk(adj, v, L, 1.0 / p, 1.0 / q, outs) for v in starts]
    state = np.random.get_state()
    np.random.seed(321)
    got = s.single_walks(starts).cpu().numpy()
    assert _state_equal(np.random.get_state(), state)
    assert got.tolist() == [w[1:] for w in want]
    stood = {int(v) for w in want for v in w[1:-1]}
    assert set(range(info["nhub"])) <= stood


def test_too_many_entries_for_the_counting_is_said_in_python(long_graph):
    from pinsage_hip import sampling
    g = long_graph[0]
    lim = sampling.paths_topk_max_entries()
    with pytest.raises(ValueError, match=str(lim)):
        sampling.walk_sample(g, [8, 9], 5, W=lim // 2 + 1, L=2, rng="philox", p=2.0)
    assert sampling.walk_sample(g, [8, 9], 5, W=lim // 2, L=2, rng="philox", p=2.0).B == 2


# ---------------------------------------------------------------------------------------------------------------- 5. surface

def test_bad_p_and_q_are_refused(graphs):
    from pinsage_hip import sampling
    from utils.random_walk import RandomWalkSampler
    g = graphs[False][0]
    ei, w = bc.case_graph()[:2]
    for kw in ({"p": 0}, {"q": -1}, {"p": float("inf")}, {"q": float("inf")}, {"p": float("nan")}, {"q": float("nan")},
               {"p": 1.0, "q": 0.0}, {"p": 1e-320}):
        with pytest.raises(ValueError, match="finite"):
            RandomWalkSampler.from_graph(g, **kw)
        with pytest.raises(ValueError, match="finite"):
            RandomWalkSampler(torch.from_numpy(ei), torch.from_numpy(w), **kw)
        with pytest.raises(ValueError, match="finite"):
            sampling.walk_paths(g, [0], 2, rng="philox", **kw)
        with pytest.raises(ValueError, match="finite"):
            sampling.walk_sample(g, [0], 5, rng="philox", **kw)


def test_sinks_need_philox(graphs):
    from utils.random_walk import RandomWalkSampler
    g, adj, outs, info, V = graphs[True]
    s = RandomWalkSampler.from_graph(g, walk_length=3, num_walks=10, p=0.25, q=4.0)
    for call in (lambda: s.single_walks([1, 2]), lambda: s.sample_batch([1, 2], 5), lambda: s.sample_batches([1, 2], 5, layers=2),
                 lambda: s._single_walk(1), lambda: s.batch_sample_neighbors([1], 5)):
        with pytest.raises(NotImplementedError, match="[Pp]hilox"):
            call()
    # the unbiased sampler still serves that graph with rng='numpy'
    assert RandomWalkSampler.from_graph(g, walk_length=3, num_walks=10).sample_batch([1, 2], 5).B == 2
    ph = RandomWalkSampler.from_graph(g, walk_length=3, num_walks=10, rng="philox", seed=11, p=0.25, q=4.0)
    starts = np.concatenate([np.repeat(np.arange(V), 4), info["sink"][:4]])
    paths = ph.single_walks(starts).cpu().numpy()
    sink = set(info["sink"].tolist())
    stopped = 0
    for s0, path in zip(starts.tolist(), paths.tolist()):
        cur = s0
        for st, x in enumerate(path):
            if cur in sink:
                assert all(y == -1 for y in path[st:])           # -1 from the sink on
                stopped += 1
                break
            assert x in outs[cur]                                 # every step follows an edge
            cur = x
    assert stopped > 20 and (paths[-4:] == -1).all()
    batch = ph.sample_batch(starts[-6:], 7)
    assert batch.nvalid.tolist()[-4:] == [0, 0, 0, 0] and batch.nvalid.tolist()[0] > 0


def test_from_graph_and_constructor_agree(graphs):
    from utils.random_walk import RandomWalkSampler
    g, _, _, info, _ = graphs[False]
    ei, w = bc.case_graph()[:2]
    a = RandomWalkSampler.from_graph(g, walk_length=3, num_walks=9, p=0.5, q=2.0)
    b = RandomWalkSampler(torch.from_numpy(ei), torch.from_numpy(w), 3, 9, 0.5, 2.0)
    assert (a.p, a.q, b.p, b.q) == (0.5, 2.0, 0.5, 2.0)
    nodes = _case_nodes(info)
    np.random.seed(5)
    x = a.sample_batch(nodes, 6)
    np.random.seed(5)
    y = b.sample_batch(nodes, 6)
    assert torch.equal(x.ids, y.ids) and torch.equal(x.counts, y.counts) and torch.equal(x.nvalid, y.nvalid)


def test_hard_negatives_follow_the_bias(graphs):
    from data.negative_sampler import NegativeSampler
    from utils.random_walk import RandomWalkSampler
    g, adj, _, info, V = graphs[False]
    p, q = 0.25, 4.0
    s = RandomWalkSampler.from_graph(g, walk_length=2, num_walks=100, p=p, q=q)

    class _Dataset:
        movie_id_to_idx = {1000 + i: i for i in range(V - 40)}

    ns = NegativeSampler(_Dataset(), random_walk_sampler=s)
    queries = _case_nodes(info)[:8]
    for nh, mx, mn in ((5, 12, 2), (4, 3, 1), (5, 5000, 2000)):                  # a window, a short window, the empty default
        np.random.seed(41)
        want = bc.hard_negatives(adj, V - 40, queries, 2, 1.0 / p, 1.0 / q, nh, mx, mn)
        state = np.random.get_state()
        np.random.seed(41)
        got = ns.sample_hard_negatives(torch.tensor(queries), num_hard_samples=nh, max_rank=mx, min_rank=mn)
        assert np.array_equal(got.numpy(), want) and _state_equal(np.random.get_state(), state)
    # the unbiased restatement gives other negatives for the window
    np.random.seed(41)
    plain = bc.hard_negatives(adj, V - 40, queries, 2, 1.0, 1.0, 5, 12, 2)
    np.random.seed(41)
    assert not np.array_equal(plain, bc.hard_negatives(adj, V - 40, queries, 2, 1.0 / p, 1.0 / q, 5, 12, 2))


def test_sharded_pipeline_refuses_a_biased_sampler(graphs):
    from pinsage_hip import shard
    from utils.random_walk import RandomWalkSampler
    g = graphs[False][0]
    biased = RandomWalkSampler.from_graph(g, p=0.5, q=1.0)
    with pytest.raises(ValueError, match="biased"):
        shard.ShardedPinSage({}, 2, biased, 10, standin=(0, 1))
    ops = shard.HipOps()
    with pytest.raises(ValueError, match="biased"):
        ops.sample(biased, torch.arange(4).cuda(), 5)
    with pytest.raises(ValueError, match="biased"):
        ops.sample_layers(biased, 0, 4, 5, 2)
    plain = RandomWalkSampler.from_graph(g, rng="philox")
    assert ops.sample(plain, torch.arange(4).cuda(), 5).B == 4


def test_the_default_sampler_runs_the_existing_path(monkeypatch):
    from pinsage_hip import native as nv
    from utils.random_walk import RandomWalkSampler
    ei, w = bc.case_graph()[:2]
    s = RandomWalkSampler(torch.from_numpy(ei), torch.from_numpy(w), walk_length=2, num_walks=20)
    names = []
    real = nv.call
    monkeypatch.setattr(nv, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    np.random.seed(1)
    s.sample_batch([1, 2, 3], 5)
    s.sample_batches([1, 2, 3], 5, layers=2)
    s.single_walks([1, 2, 3])
    s.batch_sample_neighbors([4], 5)
    assert s.graph.nbr_sorted is None
    assert "ps_walk_paths_biased" not in names and "ps_paths_topk" not in names
    assert {"ps_walk_sample", "ps_walk_sample_layers", "ps_walk_paths"} <= set(names)
    # a compacted graph cannot walk biased, and says so
    b = RandomWalkSampler.from_graph(s.graph, rng="philox", p=2.0)
    assert b.sample_batch([1], 3).B == 1 and s.graph.nbr_sorted is not None
    s.graph.compact()
    assert s.graph.nbr_sorted is None                             # dropped with the arrays it goes with
    with pytest.raises(ValueError, match="wsorted"):
        b.sample_batch([1], 3)
    s.graph.expand()                                              # col / cdf / guide come back, the sorted weights do not
    with pytest.raises(ValueError, match="wsorted"):
        b.sample_batch([1], 3)


# ------------------------------------------------------------------------------------------------------------ 6. C ABI contract

GUARD = 64


def _guarded(shape, dtype=torch.int32):
    n = int(np.prod(shape))
    raw = torch.full((n + 2 * GUARD,), -12345, dtype=dtype, device="cuda")
    return raw, raw[GUARD:GUARD + n].view(shape)


def _guards_intact(raw):
    return bool((raw[:GUARD] == -12345).all()) and bool((raw[-GUARD:] == -12345).all())


def test_abi_contract_of_the_biased_walk(graphs):
    from pinsage_hip import native as nv
    g, adj, outs, _, V = graphs[True]
    lib = nv.lib()
    null, st = ctypes.c_void_p(0), nv.stream()
    assert lib.ps_walk_paths_biased(null, null, null, null, null, 0, null, 0, 2, nv.PS_RNG_PHILOX, null, null, 0, 0, 0, null, null, st) == nv.PS_OK
    starts = _dev([0, 5, -1, V, 17, 2 ** 40, 30], np.int64)
    B, L = starts.numel(), 3
    bias = _dev([4.0, 0.25])
    raw, paths = _guarded((B, L))
    ptrs = dict(rowptr=g.rowptr, col=g.col, w=g.wsorted, cdf=g.cdf, nbr=g.sorted_neighbors(), starts=starts, bias=bias, paths=paths)

    def call(L_=L, mode=nv.PS_RNG_PHILOX, **over):
        a = {k: nv.ptr(v) for k, v in ptrs.items()}
        a.update({k: nv.ptr(v) for k, v in over.items()})
        return lib.ps_walk_paths_biased(a["rowptr"], a["col"], a["w"], a["cdf"], a["nbr"], V, a["starts"], B, L_, mode,
                                        a.get("uniforms", null), a.get("uoff", null), 7, 0, 0, a["bias"], a["paths"], st)

    for k in ptrs:
        assert call(**{k: None}) == nv.PS_EINVAL, k
    assert call(L_=0) == nv.PS_EINVAL and call(L_=-1) == nv.PS_EINVAL
    assert call(mode=nv.PS_RNG_STREAM) == nv.PS_EINVAL and call(mode=nv.PS_RNG_STREAM_RAW) == nv.PS_EINVAL       # no uniforms
    torch.cuda.synchronize()
    assert bool((raw == -12345).all())                            # a refused call writes nothing
    assert call() == nv.PS_OK
    torch.cuda.synchronize()
    got = paths.cpu().numpy()
    assert _guards_intact(raw)
    assert (got[[2, 3, 5]] == -1).all() and (got[[0, 1, 4, 6], 0] >= 0).all()      # starts outside the graph are isolated nodes
    # a bias that is not finite and positive: no walk moves (see the module docstring)
    for bad in ([0.0, 1.0], [1.0, -1.0], [float("inf"), 1.0], [1.0, float("nan")]):
        paths.fill_(3)
        assert call(bias=_dev(bad)) == nv.PS_OK
        torch.cuda.synchronize()
        assert bool((paths == -1).all()) and _guards_intact(raw)


def test_abi_contract_of_paths_topk():
    from pinsage_hip import native as nv
    lib = nv.lib()
    null, st = ctypes.c_void_p(0), nv.stream()
    assert lib.ps_paths_topk(null, 0, 8, 3, null, null, null, st) == nv.PS_OK
    lim = lib.ps_paths_topk_max_entries()
    assert lim >= 4096
    B, n, T = 5, 37, 9
    rs = np.random.RandomState(3)
    host = rs.randint(-1, 6, size=(B, n)).astype(np.int32)
    host[2] = -1
    paths = _dev(host)
    raws, outs = zip(*[_guarded((B, T)), _guarded((B, T)), _guarded((B,))])
    ids, counts, nvalid = outs
    assert lib.ps_paths_topk(null, B, n, T, nv.ptr(ids), nv.ptr(counts), nv.ptr(nvalid), st) == nv.PS_EINVAL
    assert lib.ps_paths_topk(nv.ptr(paths), B, n, T, null, nv.ptr(counts), nv.ptr(nvalid), st) == nv.PS_EINVAL
    assert lib.ps_paths_topk(nv.ptr(paths), B, n, T, nv.ptr(ids), null, nv.ptr(nvalid), st) == nv.PS_EINVAL
    assert lib.ps_paths_topk(nv.ptr(paths), B, n, T, nv.ptr(ids), nv.ptr(counts), null, st) == nv.PS_EINVAL
    assert lib.ps_paths_topk(nv.ptr(paths), B, n, 0, nv.ptr(ids), nv.ptr(counts), nv.ptr(nvalid), st) == nv.PS_EINVAL
    assert lib.ps_paths_topk(nv.ptr(paths), B, 0, T, nv.ptr(ids), nv.ptr(counts), nv.ptr(nvalid), st) == nv.PS_EINVAL
    assert lib.ps_paths_topk(nv.ptr(paths), B, lim + 1, T, nv.ptr(ids), nv.ptr(counts), nv.ptr(nvalid), st) == nv.PS_EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((r == -12345).all()) for r in raws)
    assert lib.ps_paths_topk(nv.ptr(paths), B, n, T, nv.ptr(ids), nv.ptr(counts), nv.ptr(nvalid), st) == nv.PS_OK
    torch.cuda.synchronize()
    assert all(_guards_intact(r) for r in raws)
    wi, wc, wn = bc.topk_from_paths(host, T)
    assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(counts.cpu().numpy(), wc) and np.array_equal(nvalid.cpu().numpy(), wn)
    assert wn.max() < T and wn[2] == 0                            # every row is padded: -1 / 0 past nvalid
    for i in range(B):
        assert (wi[i, wn[i]:] == -1).all() and (wc[i, wn[i]:] == 0).all()
    # the largest supported row: 4096 entries, every id different, then every id the same
    big = np.stack([rs.permutation(10 ** 6)[:lim], np.full(lim, 42)]).astype(np.int32)
    from pinsage_hip import sampling
    got = sampling.paths_topk(_dev(big), lim)
    assert got.ids[0].cpu().numpy().tolist() == big[0].tolist() and got.nvalid.tolist() == [lim, 1]
    assert got.counts[1, 0].item() == lim and got.ids[1, 0].item() == 42 and bool((got.ids[1, 1:] == -1).all())

