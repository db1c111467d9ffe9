"""The walk sampler's count and select phases on planted walks (tests/helpers/select_cases.py): counts on every bitmap word
boundary up to 4096, tie classes cut by T at every position, first-visit orders that are no other order, probe chains that wrap
at the tightest load, every position-slot count full and with one lane, holes left by sinks, fused rounds that reuse the table.
tests/test_select_cases.py proves on the CPU that each case reaches its situation; here ids, counts and nvalid of every case at
every T must equal the reference's Counter / sorted / [:T] and the C oracle, bit for bit, in every form of the launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import select_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

_graphs = {}


def _device_graph(sinks):
    """DeviceGraph of the case graph (half records, destination records); its CSR / CDF == the host's"""
    from pinsage_hip.graph import DeviceGraph
    if sinks not in _graphs:
        cg, ei, ew = sc.case_graph(sinks)
        g = DeviceGraph(torch.from_numpy(ei), torch.from_numpy(ew), buckets="half", dest_info=True)
        assert g.V == cg.V == sc.V and g.has_reachable_sink == sinks and g.dest_info is not None
        assert np.array_equal(g.rowptr.cpu().numpy(), cg.rowptr) and np.array_equal(g.col.cpu().numpy(), cg.col)
        assert np.array_equal(g.cdf.cpu().numpy(), cg.cdf)
        _graphs[sinks] = g
    return _graphs[sinks]


def _assert_batch(b, want, cases, what):
    """ids / counts / nvalid of a NeighborBatch == want, naming the first case that differs"""
    got = (b.ids.cpu().numpy().astype(np.int64), b.counts.cpu().numpy(), b.nvalid.cpu().numpy())
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1] != want[1]).any(axis=1) | (got[2] != want[2]))
    if bad.size:
        i = int(bad[0])
        name = "a start node that does not walk" if cases[i] is sc.EMPTY else cases[i].name
        t = np.flatnonzero((got[0][i] != want[0][i]) | (got[1][i] != want[1][i]))
        at = f"rank {t[0]}: got ({got[0][i][t[0]]}, {got[1][i][t[0]]}) want ({want[0][i][t[0]]}, {want[1][i][t[0]]})" if t.size else \
            f"nvalid {got[2][i]} want {want[2][i]}"
        raise AssertionError(f"{what}: {bad.size} of {len(cases)} rows differ, first: case {name} (row {i}), {at}")


def _starts(cases, fill):
    """start node per entry; the entries that do not walk take their ids from `fill` in turn"""
    fill = iter(fill)
    return np.asarray([next(fill) if c is sc.EMPTY else c.start for c in cases], dtype=np.int64)


def _want(cases, nodes, T, sinks=False):
    """the reference's words, after they were held to the C oracle on the same uniforms"""
    want = sc.expected_batch(cases, T)
    o = sc.oracle_batch(cases, nodes, T, sinks)
    assert np.array_equal(o[0], want[0]) and np.array_equal(o[1], want[1]) and np.array_equal(o[2], want[2]), T
    return want


FORMS = [("default", {}), ("no destination records", dict(use_dest=False)), ("no bucket records", dict(use_buckets=False))]


@pytest.mark.parametrize("W,L", [s[:2] for s in sc.SHAPES if not s[2]])
def test_every_case_at_every_T(W, L):
    from pinsage_hip import sampling
    g = _device_graph(False)
    cases = sc.shape_cases(W, L)
    nodes = _starts(cases, ())
    u = torch.from_numpy(sc.stream(cases)).cuda()
    for T in sc.shape_T(W, L):
        want = _want(cases, nodes, T)
        for name, kw in FORMS:
            _assert_batch(sampling.walk_sample(g, nodes, T, W, L, rng="numpy", uniforms=u, **kw), want, cases, f"{name} W={W} L={L} T={T}")


@pytest.mark.parametrize("W,L", [s[:2] for s in sc.SHAPES if s[2]])
def test_sink_cases_at_every_T(W, L):
    """PS_RNG_STREAM_WALKS: per-walk stream positions by fixpoint; the walks that stop leave holes in the position buffer"""
    from pinsage_hip import sampling
    g = _device_graph(True)
    cases = sc.shape_cases(W, L, True)
    cases = cases[:1] + [sc.EMPTY] + cases[1:]                              # an isolated start node consumes nothing
    nodes = _starts(cases, sc.ISOLATED)
    planted = sc.stream(cases, sequential=True)
    host = np.concatenate([planted, np.full(len(cases) * W * L + 8 - planted.size, 0.5)])     # room for the fixpoint's first guess
    u = torch.from_numpy(host).cuda()
    for T in sc.shape_T(W, L, True):
        want = _want(cases, nodes, T, True)
        for name, kw in FORMS[:2]:
            _assert_batch(sampling.walk_sample(g, nodes, T, W, L, rng="numpy", uniforms=u, **kw), want, cases, f"sink {name} W={W} L={L} T={T}")


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("layers", [2, 3, 8])
@pytest.mark.parametrize("W,L", list(sc.FUSED))
def test_fused_rounds_reuse_the_table(W, L, layers, split, monkeypatch):
    """ps_walk_sample_layers, one wave per node (PS_WALK_SPLIT=0) and one per (node, round) (1): a round of heavy collisions,
    then a round on one node, then a round of distinct nodes, on one start row; a second start node runs them one round ahead,
    an isolated node sits between.  Every round == its single call == the reference's words."""
    from pinsage_hip import sampling
    monkeypatch.setenv("PS_WALK_SPLIT", split)
    g = _device_graph(False)
    kinds = [sc.CASES[sc.FUSED[(W, L)] + s] for s in ("_heavy", "_one", "_distinct")]
    rounds = [[kinds[r % 3], sc.EMPTY, kinds[(r + 1) % 3]] for r in range(layers)]
    nodes = _starts(rounds[0], sc.ISOLATED)
    stride = 2 * W * L
    u = torch.from_numpy(np.concatenate([sc.stream(cases) for cases in rounds])).cuda()
    assert u.numel() == layers * stride
    for T in (1, 10, W * L, W * L + 7):
        many = sampling.walk_sample_layers(g, nodes, T, layers, W, L, rng="numpy", uniforms=u)
        for r, cases in enumerate(rounds):
            one = sampling.walk_sample(g, nodes, T, W, L, rng="numpy", uniforms=u[r * stride:])
            assert torch.equal(many[r].ids, one.ids) and torch.equal(many[r].counts, one.counts) and torch.equal(many[r].nvalid, one.nvalid), \
                f"round {r} of {layers} differs from its single call, split={split} T={T}"
            _assert_batch(many[r], _want(cases, nodes, T), cases, f"round {r} of {layers} split={split} W={W} L={L} T={T}")


@pytest.mark.parametrize("W,L", [(100, 2), (409, 1)])
def test_start_nodes_that_do_not_walk(W, L):
    """isolated start nodes and out-of-range ids (-1 and V, which only a device tensor can carry) between the others: -1 / 0 / 0
    rows, no uniforms consumed, the neighbouring rows as they were"""
    from pinsage_hip import sampling
    g = _device_graph(False)
    cases = []
    for c in sc.shape_cases(W, L):
        cases += [sc.EMPTY, c, sc.EMPTY]
    cases.append(sc.EMPTY)
    odd = [sc.ISOLATED[0], -1, sc.V, sc.ISOLATED[3], sc.V, -1] * len(cases)
    nodes = _starts(cases, odd)
    assert (nodes == -1).any() and (nodes == sc.V).any() and np.isin(sc.ISOLATED[0], nodes)
    in_range = np.where((nodes < 0) | (nodes >= sc.V), sc.ISOLATED[1], nodes)     # the oracle refuses the others, as the reference does
    u = torch.from_numpy(sc.stream(cases)).cuda()
    dev_nodes = torch.from_numpy(nodes).cuda()
    for T in (1, 10, W * L, W * L + 7):
        want = _want(cases, in_range, T)
        for name, kw in FORMS:
            _assert_batch(sampling.walk_sample(g, dev_nodes, T, W, L, rng="numpy", uniforms=u, **kw), want, cases, f"{name} W={W} L={L} T={T}")


@pytest.mark.parametrize("B", [1, 65536, 65537, 2 * 65536 + 1024 + 5])
def test_uniform_offsets_over_more_than_one_pass(B):
    """ps_uniform_offsets: one block, 64 x 1024 start nodes per pass, the count carried between passes"""
    from pinsage_hip import native as nv
    W, L = 3, 2
    deg = np.array([2, 0, 1, 0, 3], dtype=np.int64)
    V = deg.size
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    starts = np.random.RandomState(B % 1000).randint(-1, V + 1, size=B).astype(np.int64)      # -1 and V: out of range
    starts[-1] = 4
    if B > 65536:
        starts[65530:65536] = [0, 1, -1, V, 2, 4]                           # the last nodes of the first pass
        starts[65536] = 4                                                   # the first of the second
    ok = (starts >= 0) & (starts < V)
    active = np.zeros(B, dtype=np.int64)
    active[ok] = deg[starts[ok]] > 0
    dev = torch.device("cuda:0")
    uoff = torch.full((B,), -7, dtype=torch.int64, device=dev)
    total = torch.full((1,), -7, dtype=torch.int64, device=dev)
    d_rowptr, d_starts = torch.from_numpy(rowptr).to(dev), torch.from_numpy(starts).to(dev)
    with torch.cuda.device(dev):
        nv.call("ps_uniform_offsets", nv.ptr(d_rowptr), V, nv.ptr(d_starts), B, W, L, nv.ptr(uoff), nv.ptr(total), nv.stream())
    assert np.array_equal(uoff.cpu().numpy(), W * L * (np.cumsum(active) - active))
    assert int(total.item()) == W * L * int(active.sum())
