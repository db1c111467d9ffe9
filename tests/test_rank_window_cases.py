"""tests/helpers/rank_window_cases.py on the CPU: the two restatements of ps_rank_window agree on every case, every case has the
property each of its tags names, the pick rule returns distinct members of the window and gives every subset equal mass, the
host fill of pinsage_hip.negatives is held to a hand-worked row, and the python surface that needs no device is in place."""
import itertools

import numpy as np
import pytest

from helpers import rank_window_cases as rw


@pytest.mark.parametrize("name", rw.NAMES)
def test_restatement_equals_brute_force(name):
    c = rw.case(name)
    window, nwin, picks = rw.expected(name)
    bw, bn = rw.brute(c.score, c.limit, c.skip, c.lo, c.hi)
    assert np.array_equal(window, bw) and np.array_equal(nwin, bn)
    assert window.shape == (c.S, c.hi - c.lo) and window.dtype == nwin.dtype == np.int32
    for s in range(c.S):                                          # ascending ids, then pads, nothing from beyond the limit
        m = int(nwin[s])
        assert (np.diff(window[s, :m]) > 0).all() and (window[s, m:] == -1).all() and (window[s, :m] < c.limit).all()
        assert c.skip is None or int(c.skip[s]) not in window[s, :m].tolist()


@pytest.mark.parametrize("name", rw.NAMES)
def test_every_case_reaches_the_branch_it_names(name):
    c = rw.case(name)
    assert c.tags
    for row, tag in c.tags:
        try:
            rw.check_tag(c, row, tag)
        except AssertionError as e:
            raise AssertionError(f"{name}: row {row} is not {tag!r}") from e
    assert c.ld > c.Vp and (c.score[:, c.Vp:] == rw.HUGE).all()   # huge scores in the pad columns of every case


def test_the_table_covers_what_it_says():
    cs = rw.cases()
    tags = {t for c in cs for _, t in c.tags}
    want = {"zeros", "salted", "below_lo", "exact_lo", "between", "exact_hi", "above_hi", "one_value", "tie_lo_only", "tie_hi_only",
            "tie_both", "skip_rank0", "skip_in_window", "skip_in_tie", "skip_minus1", "skip_beyond", "planted_beyond_limit",
            "max_window", "S1", "S3", "S70", "nwin0", "n_above_nwin", "u0", "u_max", "u_clamped", "u_neg_nan", "collision"}
    assert want | {f"byte_{b}" for b in range(8)} <= tags
    assert {c.Vp for c in cs} >= set(rw.VPS) and {c.S for c in cs} >= {1, 3, 70}
    assert any(c.lo == 0 for c in cs) and any(c.hi - c.lo == 1 for c in cs) and any(c.hi - c.lo == rw.MAX_WINDOW for c in cs)
    assert {c.n for c in cs} >= {0, 1, 6, 64}
    assert any(c.skip is None for c in cs) and any(c.skip is not None for c in cs)
    assert any(c.max_target < 0 for c in cs) and any(0 <= c.max_target < c.Vp for c in cs)
    assert rw.VPS[-1] > 65536
    # every size of the size family meets a row below, at, inside and above the window
    for Vp in rw.VPS[1:]:
        assert {t for _, t in rw.case(f"sizes-{Vp}").tags} >= {"zeros", "below_lo", "exact_lo", "between", "exact_hi", "above_hi", "salted"}
    assert sum(c.score.nbytes for c in cs) < 32 << 20


@pytest.mark.parametrize("name", [n for n in rw.NAMES if rw.case(n).n])
def test_picks_are_distinct_members_of_the_window(name):
    c = rw.case(name)
    window, nwin, picks = rw.expected(name)
    assert picks.shape == (c.S, c.n) and picks.dtype == np.int32
    for s in range(c.S):
        m, k = int(nwin[s]), min(c.n, int(nwin[s]))
        got = picks[s, :k].tolist()
        assert len(set(got)) == k and set(got) <= set(window[s, :m].tolist()) and (picks[s, k:] == -1).all()
        if m <= c.n:
            assert sorted(got) == window[s, :m].tolist()          # a window no larger than n is taken whole


def test_pick_rule_gives_every_subset_equal_mass():
    """m = 4, c = 2 over a 12 x 12 grid of cell midpoints: each of the six subsets comes up 24 times"""
    grid = (np.arange(12) + 0.5) / 12
    seen = {}
    for a, b in itertools.product(grid, grid):
        pos = rw.pick_positions(4, np.array([a, b]), 2)[0]
        assert len(set(pos)) == 2
        seen[frozenset(pos)] = seen.get(frozenset(pos), 0) + 1
    assert len(seen) == 6 and set(seen.values()) == {24}


def test_pick_rule_by_hand():
    # m = 5, n = 3: j = 2, 3, 4.  u = .5 -> t = floor(1.5) = 1; u = .3 -> floor(1.2) = 1, taken -> 3; u = .99 -> floor(4.95) = 4
    assert rw.pick_positions(5, np.array([0.5, 0.3, 0.99]), 3)[0] == [1, 3, 4]
    # n > m: c = m, j = 0, 1: every position comes out
    assert sorted(rw.pick_positions(2, np.array([0.7, 0.1, 0.4]), 3)[0]) == [0, 1]
    assert rw.pick_positions(0, np.array([0.7]), 1)[0] == []
    w = np.array([[4, 9, 11, -1]], np.int32)
    assert rw.pick(w, np.array([3], np.int32), np.array([[0.0, 0.0, 0.0, 0.5]]), 4).tolist() == [[4, 9, 11, -1]]


def test_fill_short_rows_by_hand():
    from pinsage_hip import negatives
    M = 10
    picks = np.array([[7, -1, -1, -1],           # u2 -> 7 (an earlier slot) -> 8;  9 (the query) -> 0 (wraps at M);  8 -> 9 -> 0 -> 1
                      [-1, -1, -1, -1],          # .0 -> 0;  .05 -> 0 -> 1;  .999.. -> 9;  .95 -> 9 -> 0 -> 1 -> 2
                      [3, 4, 5, 6]])             # nothing to fill
    queries = np.array([9, 5, 0])
    u2 = np.array([[0.5, 0.75, 0.95, 0.85], [0.0, 0.05, rw.U_MAX, 0.95], [0.1, 0.2, 0.3, 0.4]])
    want = [[7, 8, 0, 1], [0, 1, 9, 2], [3, 4, 5, 6]]
    for fn in (negatives.fill_short_rows, rw.fill_short_rows):
        out = fn(picks, queries, u2, M)
        assert out.dtype == np.int64 and out.tolist() == want
        for b in range(3):
            assert len(set(out[b].tolist())) == 4 and queries[b] not in out[b]
        with pytest.raises(ValueError):
            fn(picks, queries, u2, 5)            # M = n + 1: the query and four distinct slots do not fit
    assert picks[0, 1] == -1                     # the argument is left alone
    rs = np.random.RandomState(5)
    p = np.where(np.arange(6)[None, :] < rs.randint(0, 7, 40)[:, None], rs.permutation(240).reshape(40, 6) % 30 + 30, -1)
    q, u = rs.randint(0, 60, 40), rs.random_sample((40, 6))
    a, b = negatives.fill_short_rows(p, q, u, 60), rw.fill_short_rows(p, q, u, 60)
    assert np.array_equal(a, b) and ((a >= 0) & (a < 60)).all() and np.array_equal(a[p >= 0], p[p >= 0])


def test_python_surface():
    import inspect

    from data.negative_sampler import NegativeSampler
    from pinsage_hip import native, negatives, ppr
    from utils.random_walk import RandomWalkSampler
    assert native.PROTOTYPES["ps_rank_window_max"] == "i" and native.PROTOTYPES["ps_rank_window"] == "i pqqqqpqqpipppp"
    assert NegativeSampler.hard_method == "walk"
    sig = inspect.signature(ppr.ppr_rank_window)
    assert list(sig.parameters)[:4] == ["graph", "sources", "lo", "hi"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(
        n=0, uniforms=None, alpha=0.15, sweeps=10, max_target=None, skip_self=True, source_chunk=None, skip_rows=True)
    assert list(inspect.signature(RandomWalkSampler.ppr_rank_window).parameters) == ["self", "nodes", "min_rank", "max_rank", "kw"]
    assert list(inspect.signature(negatives.sample_hard_negatives_ppr).parameters) == \
        ["sampler", "num_movies", "query_indices", "num_hard_samples", "max_rank", "min_rank"]
    assert list(inspect.signature(negatives.fill_short_rows).parameters) == ["picks", "queries", "u2", "num_movies"]

    class _Dataset:
        movie_id_to_idx = {i: i for i in range(20)}

    import torch
    s = NegativeSampler(_Dataset(), random_walk_sampler=object())
    s.hard_method = "pagerank"
    with pytest.raises(ValueError, match="hard_method"):
        s.sample_hard_negatives(torch.arange(3))
    # an empty or inverted window makes no device call: every slot is the fill's, 2 B n doubles are drawn
    s.hard_method = "ppr"
    for mn, mx in ((5, 5), (9, 2)):
        np.random.seed(3)
        out = s.sample_hard_negatives(torch.tensor([4, 0, 19]), num_hard_samples=4, max_rank=mx, min_rank=mn)
        fresh = np.random.RandomState(3)
        fresh.random_sample((3, 4))
        want = rw.fill_short_rows(np.full((3, 4), -1), [4, 0, 19], fresh.random_sample((3, 4)), 20)
        assert out.dtype == torch.int64 and out.tolist() == want.tolist()
        assert np.random.random_sample() == fresh.random_sample()
