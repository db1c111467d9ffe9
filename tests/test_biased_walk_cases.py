"""tests/helpers/biased_walk_cases.py on the CPU: the restatement of the node2vec-biased walk against a hand-computed graph and
against the reference's plain loop, and proof that the case graph and the planted batch hold what the GPU tests
(tests/test_hip_biased_walk.py) rely on -- every out-degree of DEGREES, all three alpha classes in one row, the node whose only
out-edge returns to its predecessor, parallel edges, a self loop, a tie planted on a biased row of every degree."""
from fractions import Fraction

import numpy as np

from helpers import biased_walk_cases as bc


def test_hand_computed_probabilities():
    """0 -> 1, 2;  1 -> 0, 2, 3;  2 -> 0;  3 -> 1.  A walk that came from 0 and stands on 1 sees its row (0, 2, 3) with weights
    (1, 2, 4): 0 is the way back (1/p), 2 is a destination of 0 (1), 3 is not (1/q)."""
    adj = [[(1, 1.0), (2, 2.0)], [(0, 1.0), (2, 2.0), (3, 4.0)], [(0, 3.0)], [(1, 1.0)]]
    outs = bc.out_sets(adj)
    assert bc.alpha_classes([0, 2, 3], 0, outs).tolist() == [0, 1, 2]
    for p, q in bc.BIASES + ((3.0, 7.0),):
        dest, w = bc.biased_weights(adj, outs, 1, 0, 1.0 / p, 1.0 / q)
        assert dest == [0, 2, 3]
        assert w.tolist() == [1.0 * (1.0 / p), 2.0 * 1.0, 4.0 * (1.0 / q)]
        probs = w / w.sum()
        exact = [Fraction(1) / Fraction(p), Fraction(2), Fraction(4) / Fraction(q)]
        for got, want in zip(probs, exact):
            assert abs(Fraction(float(got)) - want / sum(exact)) < Fraction(1, 2 ** 50)
    dest, w = bc.biased_weights(adj, outs, 1, 0, 4.0, 0.25)                     # p = 0.25, q = 4
    assert (w / w.sum()).tolist() == (np.array([4.0, 2.0, 1.0]) / 7.0).tolist()
    # x == t takes precedence over "t has an out-edge to x": a self loop at t
    adj2 = [[(0, 1.0), (1, 1.0)], [(0, 2.0), (1, 1.0)]]
    assert bc.alpha_classes([0, 1], 0, bc.out_sets(adj2)).tolist() == [0, 1]
    # the first step has no previous node
    assert bc.biased_weights(adj, outs, 1, None, 4.0, 0.25)[1].tolist() == [1.0, 2.0, 4.0]
    cdf = bc.choice_cdf(w)
    assert cdf[-1] == 1.0 and np.all(np.diff(cdf) > 0)


def test_unbiased_helper_is_the_plain_loop():
    _, _, V, _, adj, outs = bc.case_graph()
    for L in (1, 2, 3):
        np.random.seed(1234 + L)
        a = [bc.single_walk(adj, s, L, 1.0, 1.0, outs) for s in range(0, V, 3)]
        sa = np.random.get_state()
        np.random.seed(1234 + L)
        b = [bc.plain_single_walk(adj, s, L) for s in range(0, V, 3)]
        sb = np.random.get_state()
        assert a == b and all(len(w) == L + 1 for w in a)
        assert np.array_equal(sa[1], sb[1]) and sa[2] == sb[2]
    # and a bias changes the walks
    np.random.seed(7)
    c = [bc.single_walk(adj, s, 3, 4.0, 0.25, outs) for s in range(0, V, 3)]
    np.random.seed(7)
    d = [bc.plain_single_walk(adj, s, 3) for s in range(0, V, 3)]
    assert c != d


def test_case_graph_holds_every_case():
    ei, w, V, info, adj, outs = bc.case_graph()
    assert 200 <= V <= 400 and w.dtype == np.float32 and ei.dtype == np.int64
    deg = np.array([len(r) for r in adj])
    assert deg.min() >= 1                                                        # no sinks
    for d in bc.DEGREES:
        assert len(info["class"][d]) == bc.REPEATS and all(deg[v] == d for v in info["class"][d])
    assert set(np.unique(w * 2).tolist()) <= set(range(1, 11))                  # ratings 0.5 .. 5.0
    # not bipartite: an odd cycle (the self loop), and triangles
    loop = info["self_loop"]
    assert loop in outs[loop]
    a, b = info["parallel"]
    assert [d for d, _ in adj[a]].count(b) >= 2
    r, t = info["returner"]
    assert [d for d, _ in adj[r]] == [t] and r in outs[t]
    # all three alpha classes in ONE row, for a row of every degree that can hold them, reached over an edge t -> v
    for d in bc.DEGREES:
        found = False
        for v in info["class"][d]:
            for t_ in range(V):
                if v in outs[t_]:
                    cls = set(bc.alpha_classes([x for x, _ in adj[v]], t_, outs).tolist())
                    found |= cls == {0, 1, 2}
        assert found == (d >= 7), d
    # the graph with sinks: the same, some ordinary nodes without out-edges, reachable
    _, _, V2, info2, adj2, _ = bc.case_graph(True)
    assert V2 == V and all(len(adj2[s]) == 0 for s in info2["sink"]) and len(info2["sink"]) > 10
    assert any(x in set(info2["sink"].tolist()) for row in adj2 for x, _ in row)


def test_planted_batch_covers_every_degree():
    _, _, V, info, adj, outs = bc.case_graph()
    p = bc.planted_paths(0.25, 4.0)
    assert p.picks.shape == (V * bc.PLANT_REPEATS, bc.PLANT_L) and (p.picks >= 0).all()
    later = p.prev >= 0
    assert later[:, 1:].all() and not later[:, 0].any()
    tie = [bc.KINDS.index(k) for k in bc.TIE_KINDS]
    for d in bc.DEGREES:
        kinds = set(p.kind[later & (p.deg == d)].tolist())
        want = {bc.KINDS.index("tie_dn")} if d == 1 else set(tie)
        assert want <= kinds, (d, kinds)
        assert {bc.KINDS.index("zero"), bc.KINDS.index("umax")} <= kinds, (d, kinds)
    r, t = info["returner"]
    assert ((p.row == r) & (p.prev == t)).any()
    # every planted uniform is one random_sample() can return, and a planted tie really is a CDF entry of the biased row
    assert (p.uniforms >= 0.0).all() and (p.uniforms <= bc.U_MAX).all()
    i, st = [int(x[0]) for x in np.nonzero(later & (p.kind == tie[0]) & (p.deg == 65))]
    _, wts = bc.biased_weights(adj, outs, int(p.row[i, st]), int(p.prev[i, st]), 4.0, 0.25)
    assert p.uniforms[i * bc.PLANT_L + st] in bc.choice_cdf(wts).tolist()
    # a planted step on a biased row differs from the same uniform on the plain row somewhere: the bias is visible
    differs = 0
    for i, st in zip(*np.nonzero(later)):
        dest, wts = bc.biased_weights(adj, outs, int(p.row[i, st]), None, 1.0, 1.0)
        k = min(int(np.searchsorted(bc.choice_cdf(wts), p.uniforms[i * bc.PLANT_L + st], side="right")), len(dest) - 1)
        differs += dest[k] != p.picks[i, st]
        if differs > 50:
            break
    assert differs > 50


def test_long_row_graph_covers_every_threshold():
    """rows on both sides of 1024 edges (products kept in LDS / recomputed), of 8192 edges (one / two buffers of numpy's sum) and
    beyond 128 chunks of 64 (the chain replayed past the kept accumulators), each stood on with a previous node and planted with
    ties, 0 and 1 - 2^-53; targets beyond edge 8192 in the rows that have them"""
    ei, w, V, info, adj, outs = bc.long_graph()
    deg = np.array([len(r) for r in adj])
    assert deg.min() >= 1 and bc.LONG_DEGREES == (1023, 1024, 1025, 8191, 8192, 8193, 8300)
    assert all(deg[info["hub"][d]] == d for d in bc.LONG_DEGREES)
    p = bc.planted_long_paths(0.25, 4.0)
    assert (p.picks >= 0).all() and (p.uniforms >= 0.0).all() and (p.uniforms <= bc.U_MAX).all()
    later = p.prev >= 0
    K = {k: i for i, k in enumerate(bc.KINDS)}
    for d in bc.LONG_DEGREES:
        on = later & (p.deg == d)
        kinds = set(p.kind[on].tolist())
        assert {K[k] for k in bc.TIE_KINDS} | {K["zero"], K["umax"], K["random"]} <= kinds, (d, kinds)
        # all three alpha classes in the row, for some previous node the planted walks came from
        v = info["hub"][d]
        assert any(set(bc.alpha_classes([x for x, _ in adj[v]], int(t), outs).tolist()) == {0, 1, 2} for t in np.unique(p.prev[on]))
        # a previous node with a long row itself: the membership search over a hub's sorted destinations
        assert (deg[p.prev[on]] >= 1023).any(), d
        tied = on & np.isin(p.kind, [K[k] for k in bc.TIE_KINDS])
        assert (p.target[tied] >= d - bc.LONG_TAIL).any() and (p.target[tied] < d - bc.LONG_TAIL).any(), d
    for d in (8193, 8300):                                            # ties in the second buffer / past the 128th chunk
        tied = later & (p.deg == d) & np.isin(p.kind, [K[k] for k in bc.TIE_KINDS])
        assert (p.target[tied] >= 8192).any(), d
