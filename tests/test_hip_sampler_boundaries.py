"""The walk sampler's CDF search on planted uniforms (tests/helpers/walk_cases.py): exact ties u == cdf[e] and their
neighbours, both ends of the half records' fp32 sliver, bucket edges u ~ j / deg, 0.0, the smallest double, 1 - 2^-53, on rows
with zero weights (duplicated CDF entries, cdf[0] == 0.0), denormal CDF entries, block-boundary degrees and buckets that hold
up to ~40 entries -- through every search form the switches allow.  tests/test_walk_cases.py proves on the CPU which branch
each planted step takes; here every form's full visit histogram (T = W * L: one wrong pick changes it) must equal the
generator's np.searchsorted walk and the C oracle's, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import walk_cases as wc  # noqa: E402
from graph_defs import check_graph_definitions  # noqa: E402

pytestmark = pytest.mark.gpu

_graphs = {}


def _device_graph(sinks, form):
    """DeviceGraph of the case graph with 32- or 64-byte records and destination records; its CSR / CDF == the host's"""
    from pinsage_hip.graph import DeviceGraph
    key = (sinks, form)
    if key not in _graphs:
        cg, info, guide, ei, ew = wc.case_graph(sinks)
        g = DeviceGraph(torch.from_numpy(ei), torch.from_numpy(ew), buckets=form, dest_info=True)
        assert g.V == cg.V and g.has_reachable_sink == sinks and g.bucket_bytes == (32 if form == "half" else 64)
        assert np.array_equal(g.rowptr.cpu().numpy(), cg.rowptr) and np.array_equal(g.col.cpu().numpy(), cg.col)
        assert np.array_equal(g.cdf.cpu().numpy(), cg.cdf)                 # zero weights and 1e-30 .. 1e10 rows included
        assert np.array_equal(g.guide.cpu().numpy(), guide)              # ties helpers/walk_cases.host_guide to the built table
        check_graph_definitions(g)                                         # node / packed / bucket / destination records of THIS graph
        _graphs[key] = g
    return _graphs[key]


def _assert_batch(b, want, what):
    ids, counts, nvalid = want
    got_ids = b.ids.cpu().numpy().astype(np.int64)
    bad = np.flatnonzero((got_ids != ids).any(axis=1) | (b.counts.cpu().numpy() != counts).any(axis=1))
    assert bad.size == 0, f"{what}: visit histogram of {bad.size} start nodes differs, first batch row {bad[0]}"
    assert np.array_equal(b.nvalid.cpu().numpy(), nvalid), what


# (name, record form of the graph, walk_sample switches).  Not 8 x 3 distinct paths: at (192, 3) the launch drops the destination
# records (more than 4 positions per lane), so the "+dest" forms run the kernels of the plain ones there and only (100, 2) and
# (1, 1) use the staged records; at (1, 1) every walk ends after step 0, so only the two hubs (start rows too long to stage)
# reach the packed blocks in global memory and the bucket records at all -- the short rows are searched in LDS in every form.
FORMS = [("bisect", "half", dict(use_guide=False)),
         ("guide", "half", dict(use_packed=False, use_buckets=False)),
         ("packed", "half", dict(use_buckets=False, use_dest=False)),
         ("packed+dest", "half", dict(use_buckets=False, use_dest=True)),
         ("full", "full", dict(use_dest=False)),
         ("full+dest", "full", dict(use_dest=True)),
         ("half", "half", dict(use_dest=False)),
         ("half+dest", "half", dict(use_dest=True))]


@pytest.mark.parametrize("W,L", wc.SHAPES)
def test_every_search_form_on_planted_uniforms(W, L):
    from oracle import c_oracle as co
    from pinsage_hip import sampling
    cg = wc.case_graph()[0]
    nodes, uoff, p = wc.planted_batch(W, L)
    T = W * L
    want = p.histogram(T)
    o = co.walk_sample(cg, nodes, T, L, W, uniforms=p.uniforms, uoff=uoff, threads=4)
    assert np.array_equal(o[0], want[0]) and np.array_equal(o[1], want[1]) and np.array_equal(o[2], want[2])
    u = torch.from_numpy(p.uniforms).cuda()
    for name, form, kw in FORMS:
        g = _device_graph(False, form)
        _assert_batch(sampling.walk_sample(g, nodes, T, W, L, rng="numpy", uniforms=u, **kw), want, f"{name} W={W} L={L}")


@pytest.mark.parametrize("W,L", wc.SHAPES)
def test_sink_graph_on_planted_uniforms(W, L):
    """PS_RNG_STREAM_WALKS: per-walk stream positions by fixpoint, half and full records; expected: the sequential C oracle"""
    from oracle import c_oracle as co
    from pinsage_hip import sampling
    sg = wc.case_graph(True)[0]
    nodes, p = wc.planted_sink_batch(W, L)
    T = W * L
    host = np.concatenate([p.uniforms, np.full(nodes.size * W * L + 8 - p.uniforms.size, 0.5)])       # room for the fixpoint's first guess
    ids, counts, nvalid, _, used, _ = co.walk_sample(sg, nodes, T, L, W, uniforms=host)
    assert used == p.uniforms.size
    want = p.histogram(T)
    assert np.array_equal(ids, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(nvalid, want[2])
    u = torch.from_numpy(host).cuda()
    for form in ("half", "full"):
        g = _device_graph(True, form)
        _assert_batch(sampling.walk_sample(g, nodes, T, W, L, rng="numpy", uniforms=u), want, f"sink {form} W={W} L={L}")
        _assert_batch(sampling.walk_sample(g, nodes, T, W, L, rng="numpy", uniforms=u, use_dest=False), want, f"sink {form} no dest W={W} L={L}")


@pytest.mark.parametrize("split", ["0", "1"])
def test_fused_layers_on_planted_uniforms(split, monkeypatch):
    """ps_walk_sample_layers, one wave per node (PS_WALK_SPLIT=0) and one per (node, layer) (1): two layers on two planted
    streams laid end to end == two separate calls == the generator"""
    from pinsage_hip import sampling
    monkeypatch.setenv("PS_WALK_SPLIT", split)
    W, L = wc.SHAPES[0]
    T = W * L
    cg = wc.case_graph()[0]
    nodes, uoff, p0 = wc.planted_batch(W, L)
    p1 = wc.plant(cg.rowptr, cg.col, cg.cdf, nodes, W, L, seed=4242, uoff=uoff)
    assert not np.array_equal(p0.uniforms, p1.uniforms)
    u = torch.from_numpy(np.concatenate([p0.uniforms, p1.uniforms])).cuda()
    for form in ("half", "full"):
        g = _device_graph(False, form)
        two = sampling.walk_sample_layers(g, nodes, T, 2, W, L, rng="numpy", uniforms=u)
        for r, p in enumerate((p0, p1)):
            one = sampling.walk_sample(g, nodes, T, W, L, rng="numpy", uniforms=u[r * p0.uniforms.size:])
            assert torch.equal(two[r].ids, one.ids) and torch.equal(two[r].counts, one.counts) and torch.equal(two[r].nvalid, one.nvalid)
            _assert_batch(two[r], p.histogram(T), f"layer {r} {form} split={split}")


@pytest.mark.parametrize("tables", [True, False])
def test_walk_paths_on_planted_uniforms(tables):
    """walk_paths_kernel's scalar search, with node records + guide and with both NULL (plain bisection): every step of every
    path == the generator's pick"""
    from pinsage_hip import native as nv
    g = _device_graph(False, "half")
    starts, uoff, p = wc.planted_paths()
    B, L = starts.size, wc.PATH_L
    dev = g.device
    st = torch.from_numpy(starts).to(dev)
    off = torch.from_numpy(uoff).to(dev)
    u = torch.from_numpy(p.uniforms).to(dev)
    paths = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nv.call("ps_walk_paths", nv.ptr(g.rowptr), nv.ptr(g.col), nv.ptr(g.cdf), nv.i64(g.V), nv.ptr(st), nv.i64(B), nv.i32(L),
                nv.i32(nv.PS_RNG_STREAM), nv.ptr(u), nv.ptr(off), nv.u64(0), nv.u32(0), nv.i32(0),
                nv.ptr(g.nodeinfo if tables else None), nv.ptr(g.guide if tables else None), nv.ptr(paths), nv.stream())
    got = paths.cpu().numpy().astype(np.int64)
    want = p.pick[:, 0, :]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{bad.shape[0]} steps differ, first: path {bad[0][0]} step {bad[0][1]} got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"
