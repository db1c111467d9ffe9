"""The planted-uniform cases of the walk sampler's CDF search (tests/helpers/walk_cases.py) prove their own coverage here,
without a GPU: which branch of each search form every planted step must take follows from the host CSR / CDF and the record
definitions, so "the tie / sliver / fifth-candidate / bisection branches are reached" is a condition on the inputs and is
asserted before tests/test_hip_sampler_boundaries.py runs the kernels on them.  The C oracle's upper_bound is pinned to
np.searchsorted(side='right') on the same uniforms, ties included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import walk_cases as wc  # noqa: E402


def test_case_graph_holds_the_rows_the_searches_need():
    cg, info, guide, ei, ew = wc.case_graph()
    rowptr, cdf = cg.rowptr, cg.cdf
    deg = np.diff(rowptr)
    assert 1000 < cg.V < 5000 and ew.dtype == np.float32
    assert bool((deg > 0).all())                                           # sink-free
    for d in (1, 2) + wc.BOUNDARY_DEGREES:
        assert int((deg == d).sum()) >= 4, d
    # start rows are either short enough to be staged in LDS or far too long, for every launch the GPU tests make
    bounds = [wc.stage_blocks(W, L, r, d) for (W, L) in wc.SHAPES for r in (1, 2) for d in (False, True)]
    assert wc.stage_blocks(100, 2) == 42 and wc.stage_blocks(100, 2, dest=True) == 28 and wc.stage_blocks(100, 2, 2, True) == 22
    assert wc.stage_blocks(192, 3, dest=True) == 96 and wc.stage_blocks(1, 1, dest=True) == 32
    assert (wc.STAGED_MAX_DEG + 6) // 8 + 1 <= min(bounds) and wc.HUB_MIN_DEG // 8 > max(bounds)
    assert not bool(((deg > wc.STAGED_MAX_DEG) & (deg < wc.HUB_MIN_DEG)).any()) and int((deg >= wc.HUB_MIN_DEG).sum()) == 2
    # rows of the block-boundary degrees start at every residue mod 8
    assert set((rowptr[info["boundary"]] & 7).tolist()) == set(range(8))
    # zero weights: a row's CDF starts at 0.0, repeats an entry in the middle, and ends in repeated 1.0s
    first, last = cdf[rowptr[:-1]], cdf[rowptr[1:] - 1]
    assert int((first == 0.0).sum()) >= 4 and bool((last == 1.0).all())
    dup = (np.diff(cdf) == 0.0) & (np.diff(np.repeat(np.arange(cg.V), deg)) == 0)
    assert int(dup.sum()) > 50 and int((dup & (cdf[:-1] == 1.0)).sum()) >= 4 and int((dup & (cdf[:-1] > 0) & (cdf[:-1] < 1)).sum()) >= 4
    # CDF entries below the smallest normal fp32: their fp32 lower bound is a denormal
    assert int(((cdf > 0) & (cdf < 2.0 ** -126)).sum()) >= 6
    # buckets that hold 3 .. 14 and ~40 entries past their guide position
    e = np.arange(cg.E)
    row = np.repeat(np.arange(cg.V), deg)
    nxt = np.where(e - rowptr[row] + 1 < deg[row], guide[np.minimum(e + 1, cg.E - 1)], deg[row])   # guide of the next bucket, row length after the last
    inside = nxt - guide
    for n in wc.CLUSTERS:
        assert bool(((inside >= n) & (inside <= n + 2)).any()), n
    # the directed copy has reachable sinks and the same constructed rows
    sg, sinfo = wc.case_graph(True)[:2]
    sdeg = np.diff(sg.rowptr)
    assert int((sdeg == 0).sum()) == sinfo["sink"].size > 100 and bool((sdeg[sg.col] == 0).any())
    assert np.array_equal(sdeg[sinfo["special"]], deg[info["special"]])


def test_the_bucket_index_clamp_cannot_be_reached_by_a_uniform():
    """`if (j >= deg) j = deg - 1` guards j = (uint32)(u * deg).  For deg in [2^k, 2^(k+1)) the doubles just below deg are
    2^(k-52) apart and deg * (1 - 2^-53) lies deg / 2^(k+1) of that spacing below deg: at least half of it, and exactly half only
    for deg = 2^k, where the product is representable (the spacing halves below a power of two).  So fl(u * deg) < deg for every
    u <= 1 - 2^-53 and the clamp is dead code for uniforms of random_sample(): no planted step can take it, and none does."""
    for d in list(range(1, 70000)) + [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1, 2 ** 32 - 1]:
        assert int(wc.U_MAX * float(d)) == d - 1
    cg, info, guide = wc.case_graph()[:3]
    for W, L in wc.SHAPES:
        p = wc.planted_batch(W, L)[2]
        t = p.taken
        assert not wc.scan_model(cg.rowptr, cg.cdf, guide, p.row[t], p.u[t], p.edge[t], packed=True)["j_clamped"].any()
        assert bool((p.u[t] == wc.U_MAX).any())


def _assert_scan_classes(sc, sel, packed, what):
    """every forward-scan length 0 .. 11 by the scan, the switch to bisection after 12 (and, in packed blocks, 13) scanned
    entries for answers 12, 13, 14 and ~40 entries past the guide position; pair and single loads"""
    s, found = sc["s"][sel], sc["found"][sel]
    for n in range(wc.LIN_PROBES):
        assert bool((found & (s == n)).any()), (what, "scan length", n)
    assert bool((~found & (sc["n_bisect"][sel] == wc.LIN_PROBES)).any()), (what, "bisection after 12 entries")
    for n in (12, 13, 14):
        assert bool((~found & (s == n)).any()), (what, "bisection, answer at", n)
    assert bool((~found & (s >= 30)).any()), (what, "deep bisection")
    assert bool((found & sc["second"][sel]).any()) and bool((found & ~sc["second"][sel]).any()), (what, "first / second entry of a pair")
    assert bool(sc["pairs"][sel].any())
    if packed:
        assert bool(sc["single7"][sel].any()), (what, "single load at slot 7")
        assert bool((sc["single7"][sel] & found).any()) and bool((sc["single7"][sel] & ~found).any())
        assert bool((found & (s == 12)).any()), (what, "a single load shifts the scan: entry 12 found without bisecting")
        assert bool((~found & (sc["n_bisect"][sel] == wc.LIN_PROBES + 1)).any()), (what, "bisection after 13 entries")
    else:
        assert not bool(sc["single7"][sel].any())


@pytest.mark.parametrize("W,L", wc.SHAPES[:2])
def test_planted_steps_reach_every_branch_of_every_search_form(W, L):
    cg, info, guide = wc.case_graph()[:3]
    nodes, uoff, p = wc.planted_batch(W, L)
    cl = wc.classify(cg.rowptr, cg.col, cg.cdf, guide, p, np.diff(cg.rowptr)[nodes])
    kind, lds = cl["kind"], cl["lds"]
    every = np.ones(kind.size, dtype=bool)
    assert bool((p.uniforms >= 0.0).all()) and bool((p.uniforms <= wc.U_MAX).all())
    for k in range(len(wc.KINDS)):
        assert int((kind == k).sum()) > 100, wc.KINDS[k]
    # lanes w and w + 64 of a start node are assigned different kinds (a kind that left [0, 1 - 2^-53] was replaced afterwards)
    assert np.gcd(wc.KIND_STRIDE, 64) == 1 and (64 * wc.KIND_STRIDE) % len(wc.KINDS) != 0
    assert float((p.kind[:, :W - 64, :] != p.kind[:, 64:, :]).mean()) > 0.9
    # ties: u == a CDF entry, at first / middle / last positions of a row, on duplicated entries and on cdf == 0.0
    tie = cl["tie"]
    lo, hi = cg.rowptr[cl["row"]], cg.rowptr[cl["row"] + 1]
    assert int(tie.sum()) > 1000
    assert bool((tie & (cl["ans"] == lo + 1)).any()) and bool((tie & (cl["ans"] == hi - 1)).any())
    assert bool((tie & (cl["u"] == 0.0)).any())                            # cdf[0] == 0.0 == u: the answer skips the zero-weight edges
    assert bool((tie & (cl["ans"] - 2 >= lo) & (cg.cdf[np.maximum(cl["ans"] - 2, 0)] == cl["u"])).any())      # tie on a duplicated entry
    # form "guide" (plain arrays + guide) and "packed" (128-byte blocks): all steps; LDS copy: step 0 of the short start rows;
    # global blocks: the rest, hubs' step 0 among them
    _assert_scan_classes(cl["guide_scan"], every, False, "guide")
    _assert_scan_classes(cl["packed_scan"], lds, True, "packed, LDS")
    _assert_scan_classes(cl["packed_scan"], ~lds, True, "packed, global")
    assert bool((~lds & (cl["st"] == 0)).any())
    # the record forms serve every step that is not searched in LDS
    full, half = cl["full"][~lds], cl["half"][~lds]
    for c in (1, 2, 3, 4, 5, 6):
        assert bool((full == c).any()), ("64-byte records", c)
    for c in (1, 2, 3, 4, 11, 12, 13, 14, 6):
        assert bool((half == c).any()), ("32-byte records", c)
    # where a wrong comparison would change the visited node: a tie u == c_i on each of the five candidates of a 64-byte record
    # (`>=` for `>` in bucket_pick or on the fifth candidate), and a tie on a CDF entry that fp32 holds exactly, u == l_i == c_i,
    # on each of the four candidates of a 32-byte record (`<=` for `<` against l_i in half_pick)
    for c in range(5):
        assert bool((~lds & (cl["full_tie"] == c)).any()), ("64-byte records: node-changing tie on candidate", c + 1)
    for c in range(4):
        assert bool((~lds & (cl["half_tie"] == c)).any()), ("32-byte records: node-changing exact tie on candidate", c + 1)
    # ... and their long way is the packed scan again, from the same guide position: short, at the limit, and bisecting
    for name, fb in (("full", cl["full"] == 6), ("half", cl["half"] >= 6)):
        sel = fb & ~lds
        s, found = cl["packed_scan"]["s"][sel], cl["packed_scan"]["found"][sel]
        assert bool((found & (s <= 6)).any()) and bool((found & (s >= 10)).any()) and bool((~found).any()), name
    assert bool((~lds & (cl["half"] == 11) & (cl["packed_scan"]["s"] == 0)).any())      # sliver of the first candidate: the long way ends at once
    # A-only, B-only, both, neither: lanes (w, w + 64) of one start node at one step
    allfour = {(False, False), (False, True), (True, False), (True, True)}
    assert wc.lane_pairs(cl, cl["full"] >= 5, ~lds, p.pick.shape) == allfour          # fifth candidate and beyond: inside the first ballot
    assert wc.lane_pairs(cl, cl["full"] == 6, ~lds, p.pick.shape) == allfour          # the long way: inside the second
    assert wc.lane_pairs(cl, cl["half"] >= 6, ~lds, p.pick.shape) == allfour
    # u at a bucket edge: below the fp64 value of j / deg and still in bucket j (what the guide threshold's 1 - 2^-50 allows for)
    d = (hi - lo).astype(np.float64)
    j = np.minimum((cl["u"] * d).astype(np.int64), hi - lo - 1)
    assert bool((cl["u"] < j / d).any()) and bool((cl["u"] == j / d).any())
    # the control: random uniforms reach no tie and no sliver -- the gap the planted kinds close
    rnd = kind == wc.K["random"]
    assert int(rnd.sum()) > 1000 and not bool((rnd & tie).any()) and not bool((rnd & cl["sliver"]).any())


def test_planted_paths_reach_every_branch_of_the_scalar_search():
    """walk_paths_kernel's own loop probes one entry at a time: 12 entries forward from the guide position, then bisection"""
    cg, info, guide = wc.case_graph()[:3]
    starts, uoff, p = wc.planted_paths()
    t = p.taken
    sc = wc.scan_model(cg.rowptr, cg.cdf, guide, p.row[t], p.u[t], p.edge[t], packed=False)
    for n in range(wc.LIN_PROBES):
        assert bool((sc["s"] == n).any()), n
    for n in (12, 13, 14):
        assert bool((sc["s"] == n).any()), n
    assert bool((sc["s"] >= 30).any())
    tie = (p.edge[t] > cg.rowptr[p.row[t]]) & (cg.cdf[np.maximum(p.edge[t] - 1, 0)] == p.u[t])
    assert int(tie.sum()) > 1000
    assert int((tie & (cg.col[np.maximum(p.edge[t] - 1, 0)] != cg.col[p.edge[t]])).sum()) > 1000       # `<` for `<=` visits another node


def _histogram_equals_oracle(cg, nodes, W, L, p, uoff):
    from oracle import c_oracle as co
    T = W * L
    ids, counts, nvalid = p.histogram(T)
    pad = np.concatenate([p.uniforms, np.full(8, 0.5)])
    o = co.walk_sample(cg, nodes, T, L, W, uniforms=pad, uoff=uoff, threads=1 if uoff is None else 4)
    assert np.array_equal(o[0], ids) and np.array_equal(o[1], counts) and np.array_equal(o[2], nvalid)
    return o


@pytest.mark.parametrize("W,L", wc.SHAPES)
def test_c_oracle_equals_numpy_searchsorted_on_the_planted_uniforms(W, L):
    """orc_walk_sample (upper_bound) == np.searchsorted(side='right') walked by the generator, ties included: the full visit
    histogram (T = W * L) of every start node, on the sink-free graph (per-node stream offsets) and on the graph with sinks
    (sequential consumption); the single walks of ps_walk_paths' case step by step."""
    from oracle import c_oracle as co
    cg = wc.case_graph()[0]
    nodes, uoff, p = wc.planted_batch(W, L)
    _histogram_equals_oracle(cg, nodes, W, L, p, uoff)
    sg = wc.case_graph(True)[0]
    snodes, sp = wc.planted_sink_batch(W, L)
    o = _histogram_equals_oracle(sg, snodes, W, L, sp, None)
    assert o[4] == sp.uniforms.size == int(sp.taken.sum())                 # the oracle consumed exactly the planted stream
    if L > 1:
        assert bool((~sp.taken[:, :, 0]).any()) and bool((sp.taken[:, :, 0] & ~sp.taken[:, :, L - 1]).any())      # isolated starts, stopped walks
    if (W, L) == wc.SHAPES[0]:
        starts, poff, pp = wc.planted_paths()
        for b in range(0, starts.size, 97):
            walk, pos = co.single_walk(cg, int(starts[b]), wc.PATH_L, pp.uniforms, int(poff[b]))
            assert walk[1:] == pp.pick[b, 0].tolist() and pos == poff[b] + wc.PATH_L
