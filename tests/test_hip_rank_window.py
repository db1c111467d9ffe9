"""The rank-window select on the device (csrc/rank_window.hip: ps_rank_window; pinsage_hip.ppr.ppr_rank_window;
NegativeSampler.hard_method = "ppr") against the restatements of tests/helpers/rank_window_cases.py, byte for byte.

The C ABI is called directly for the case table: every output is the middle of its own allocation of 0xFF bytes with a guard
band on either side.  tests/test_rank_window_cases.py holds the table and the restatements to each other without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import abi_cases as ac
from helpers import abi_cases_rank_window  # noqa: F401  (the entry point joins ac.CASES)
from helpers import ppr_cases as pc
from helpers import rank_window_cases as rw

pytestmark = pytest.mark.gpu
GUARD = 256


class _Out:
    """`count` int32 entries of 0xFF bytes with GUARD bytes of 0xFF on either side"""

    def __init__(self, count):
        self.nbytes = 4 * int(count)
        self.raw = torch.full((2 * GUARD + self.nbytes,), 0xFF, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + GUARD)

    def host(self, shape):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(np.int32).reshape(shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xFF).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xFF).all())

    def untouched(self):
        return bool((self.raw == 0xFF).all())


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the cases are read-only


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _call(score, Vp, max_target, skip, lo, hi, u, n, S=None, ld=None):
    """one direct call -> (status, window, nwin, picks or None); guard bands and inputs are checked here"""
    from pinsage_hip import native as nv
    rows = score.shape[0]
    S = rows if S is None else S
    ld = score.shape[1] if ld is None else ld
    d_score, d_skip, d_u = _dev(score), _dev(skip), _dev(u)
    W = hi - lo
    # arguments that must be refused size nothing: their buffers are those of a window of one rank, or of one pick
    window, nwin, picks = _Out(rows * (W if 0 < W <= rw.MAX_WINDOW else 1)), _Out(rows), _Out(rows * (n if 0 <= n <= rw.MAX_PICKS else 1))
    rc = nv.lib().ps_rank_window(_ptr(d_score), S, ld, Vp, max_target, _ptr(d_skip), lo, hi, _ptr(d_u), n, window.ptr(), nwin.ptr(),
                                 picks.ptr() if n else ctypes.c_void_p(0), nv.stream())
    torch.cuda.synchronize()
    assert window.guards_intact() and nwin.guards_intact() and picks.guards_intact(), "bytes outside an output were written"
    for t, a in ((d_score, score), (d_skip, skip), (d_u, u)):
        if a is not None:
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input was written"
    if rc != 0:
        assert window.untouched() and nwin.untouched() and picks.untouched(), f"status {rc} and an output was written"
        return rc, None, None, None
    return rc, window.host((S, W)), nwin.host((S,)), picks.host((S, n)) if n else None


def _run(c, rows=None):
    sel = slice(None) if rows is None else rows
    return _call(c.score[sel], c.Vp, c.max_target, None if c.skip is None else c.skip[sel], c.lo, c.hi,
                 None if c.u is None else c.u[sel], c.n)


def test_window_limit():
    from pinsage_hip import native as nv
    assert nv.lib().ps_rank_window_max() == rw.MAX_WINDOW >= 4096 and nv.lib().ps_abi_version() == 1


@pytest.mark.parametrize("name", rw.NAMES)
def test_cases_equal_the_restatement(name):
    c = rw.case(name)
    window, nwin, picks = rw.expected(name)
    runs = [_run(c) for _ in range(2)]
    for rc, w, m, p in runs:
        assert rc == 0
        assert m.tobytes() == nwin.tobytes(), f"nwin {m.tolist()} expected {nwin.tolist()}"
        bad = np.flatnonzero((w != window).any(axis=1))
        assert w.tobytes() == window.tobytes(), f"window differs in rows {bad[:8].tolist()}"
        if c.n:
            assert p.tobytes() == picks.tobytes(), f"picks differ in rows {np.flatnonzero((p != picks).any(axis=1))[:8].tolist()}"
        else:
            assert p is None
    assert all(a is None or a.tobytes() == b.tobytes() for a, b in zip(runs[0][1:], runs[1][1:]))      # a second call: the same bytes


@pytest.mark.parametrize("name", ["rows70", "skip", "ties-256", "picks-n6", "sizes-1025"])
def test_permuting_the_rows_permutes_the_outputs(name):
    c = rw.case(name)
    window, nwin, picks = rw.expected(name)
    perm = np.roll(np.arange(c.S)[::-1], c.S // 3)
    assert c.S > 1 and not np.array_equal(perm, np.arange(c.S))
    rc, w, m, p = _run(c, perm)
    assert rc == 0 and np.array_equal(w, window[perm]) and np.array_equal(m, nwin[perm])
    assert picks is None or np.array_equal(p, picks[perm])


# ---- real scores --------------------------------------------------------------------------------------------------------------
_samplers = {}


def _sampler(name):
    if name not in _samplers:
        from utils.random_walk import RandomWalkSampler
        ei, ew = pc.case(name)[:2]
        _samplers[name] = RandomWalkSampler(torch.from_numpy(ei.copy()), torch.from_numpy(ew.copy()), walk_length=2, num_walks=10)
    return _samplers[name]


_scores = {}


def _reference_scores(name, sources):
    """fp64[S, size] from ppr_cases' restatement of the reference's loop, made once per (graph, sources)"""
    key = (name, tuple(sources))
    if key not in _scores:
        size = pc.size_of(name, sources)
        _scores[key] = np.array([pc.reference_scores(pc.adjacency(name), size, s, pc.DEFAULT_ALPHA, pc.DEFAULT_SWEEPS) for s in sources])
        _scores[key].setflags(write=False)
    return _scores[key]


BIP_ITEMS = tuple(range(pc.BIP_M))


@pytest.mark.parametrize("lo,hi,want", [(3, 9, 6), (20, 30, 3), (25, 30, 0)])
def test_bip10_windows(lo, hi, want):
    """every item source of bip10 ranks the 23 other items when the query is skipped: a full window, a short one, an empty one"""
    from pinsage_hip import ppr
    sampler = _sampler("bip10")
    sources = list(BIP_ITEMS)
    score = _reference_scores("bip10", sources)
    assert all(len(rw.candidates(score[i], pc.BIP_M, s)) == 23 for i, s in enumerate(sources))
    # the query skipped: the restatement over the reference's scores
    window, nwin, none = sampler.ppr_rank_window(torch.tensor(sources), lo, hi, max_target=pc.BIP_M)
    ew, en = rw.restate(score, pc.BIP_M, np.array(sources), lo, hi)
    assert none is None and window.dtype == nwin.dtype == torch.int32 and window.is_cuda
    assert np.array_equal(window.cpu().numpy(), ew) and np.array_equal(nwin.cpu().numpy(), en) and (en == want).all()
    # nothing skipped: the slice of ps_ppr_topk's ranking, sorted by id
    window, nwin, _ = ppr.ppr_rank_window(sampler.graph, sources, lo, hi, max_target=pc.BIP_M, skip_self=False)
    top = sampler.ppr_batch(sources, hi, max_target=pc.BIP_M)
    ids, nvalid, window, nwin = top.ids.cpu().numpy(), top.nvalid.cpu().numpy(), window.cpu().numpy(), nwin.cpu().numpy()
    for i in range(len(sources)):
        members = sorted(ids[i, lo:max(lo, nvalid[i])].tolist())
        assert nvalid[i] == min(hi, 24) and window[i, :len(members)].tolist() == members and nwin[i] == len(members)
        assert len(members) == max(0, min(hi, 24) - lo) and (window[i, len(members):] == -1).all()
    # chunks of 64 source columns give the same rows as one chunk
    many = sources * 3
    a = ppr.ppr_rank_window(sampler.graph, many, lo, hi, max_target=pc.BIP_M, source_chunk=64)
    assert np.array_equal(a[0].cpu().numpy(), np.tile(ew, (3, 1))) and np.array_equal(a[1].cpu().numpy(), np.tile(en, 3))


def test_stars_resolve_ties_to_the_smaller_id():
    from pinsage_hip import ppr
    sampler = _sampler("stars")
    window, nwin, _ = sampler.ppr_rank_window([0], 3, 9)
    assert window.tolist() == [[4, 5, 6, 7, 8, -1]] and nwin.tolist() == [5]         # the eight leaves tie; the centre is skipped
    score = _reference_scores("stars", (0,))
    assert len(set(score[0, 1:9].tolist())) == 1 and score[0, 0] > score[0, 1] > 0
    window, nwin, _ = ppr.ppr_rank_window(sampler.graph, [0], 3, 9, skip_self=False)
    top = sampler.ppr_batch([0], 9)
    assert window.tolist() == [sorted(top.ids[0, 3:9].tolist())] == [[3, 4, 5, 6, 7, 8]] and nwin.tolist() == [6]
    ew, en = rw.restate(score, score.shape[1], np.array([0]), 3, 9)
    assert ew.tolist() == [[4, 5, 6, 7, 8, -1]] and en.tolist() == [5]


def test_python_argument_errors():
    from pinsage_hip import ppr
    g = _sampler("stars").graph
    for lo, hi in ((-1, 4), (4, 4), (5, 2), (0, rw.MAX_WINDOW + 1)):
        with pytest.raises(ValueError):
            ppr.ppr_rank_window(g, [0, 1], lo, hi)
    for kw in (dict(n=2), dict(n=2, uniforms=np.zeros((2, 3))), dict(n=2, uniforms=np.zeros((1, 2)))):
        with pytest.raises(ValueError):
            ppr.ppr_rank_window(g, [0, 1], 0, 4, **kw)
    window, nwin, picks = ppr.ppr_rank_window(g, [0, 1], 0, 4, n=2, uniforms=np.zeros((2, 2)))
    assert tuple(picks.shape) == (2, 2) and picks.dtype == torch.int32


# ---- status codes -------------------------------------------------------------------------------------------------------------
def test_status_codes_are_checked_before_anything_is_written():
    from pinsage_hip import native as nv
    c = rw.case("picks-n6")
    ok = dict(score=c.score, Vp=c.Vp, max_target=-1, skip=None, lo=c.lo, hi=c.hi, u=c.u, n=c.n)

    def status(**kw):
        return _call(**dict(ok, **kw))[0]

    assert status() == 0
    two31 = 1 << 31
    for kw in (dict(S=-1), dict(Vp=-1), dict(n=-1), dict(ld=c.Vp - 1), dict(lo=-1), dict(hi=c.lo), dict(hi=c.lo - 1), dict(S=two31),
               dict(Vp=two31, ld=two31), dict(hi=two31)):
        assert status(**kw) == nv.PS_EINVAL, kw
    assert status(u=None) == nv.PS_EINVAL                         # n > 0 without uniforms
    lib = nv.lib()
    out = [_Out(c.S * (c.hi - c.lo)), _Out(c.S), _Out(c.S * c.n)]
    d_score, d_u = _dev(c.score), _dev(c.u)

    def raw(score, window, nwin, picks, n=c.n, S=c.S, lo=c.lo, hi=c.hi, Vp=c.Vp):
        rc = lib.ps_rank_window(score, S, c.ld, Vp, -1, None, lo, hi, _ptr(d_u), n, window, nwin, picks, nv.stream())
        torch.cuda.synchronize()
        assert all(o.untouched() for o in out)
        return rc

    w, m, p = (o.ptr() for o in out)
    assert raw(None, w, m, p) == nv.PS_EINVAL and raw(_ptr(d_score), None, m, p) == nv.PS_EINVAL
    assert raw(_ptr(d_score), w, None, p) == nv.PS_EINVAL and raw(_ptr(d_score), w, m, None) == nv.PS_EINVAL
    assert raw(_ptr(d_score), w, m, p, n=65) == nv.PS_EUNSUPPORTED
    assert raw(_ptr(d_score), w, m, p, hi=c.lo + rw.MAX_WINDOW + 1) == nv.PS_EUNSUPPORTED
    assert raw(None, None, None, None, S=0) == 0                  # an empty problem: nothing is touched, whatever the pointers
    # Vp == 0: no score is needed; every row is pads
    rc, window, nwin, picks = _call(np.zeros((3, 0)), 0, -1, None, 2, 6, np.zeros((3, 2)), 2, ld=0)
    assert rc == 0 and (window == -1).all() and (nwin == 0).all() and (picks == -1).all()
    # max_target == 0: the same through the limit
    rc, window, nwin, picks = _call(c.score, c.Vp, 0, None, 0, 4, None, 0)
    assert rc == 0 and (window == -1).all() and (nwin == 0).all()
    # n == 0: picks is not touched, even when it is given
    rc = lib.ps_rank_window(_ptr(d_score), c.S, c.ld, c.Vp, -1, None, c.lo, c.hi, _ptr(d_u), 0, w, m, p, nv.stream())
    torch.cuda.synchronize()
    assert rc == 0 and out[2].untouched() and all(o.guards_intact() for o in out)
    assert np.array_equal(out[0].host((c.S, c.hi - c.lo)), rw.expected(c.name)[0])


def test_contract_matrix_holds_the_rank_window():
    """The contract matrix of tests/test_hip_abi_contract.py (captured stream, poisoned outputs, guard bands, replays) for the entry
    point, started from here as well: that module parametrises over the case table when it is collected, and a run of it alone
    does not import the case module of this entry point."""
    import test_hip_abi_contract as contract
    assert "ps_rank_window" in ac.CASES
    contract.test_contract("ps_rank_window")


# ---- NegativeSampler ----------------------------------------------------------------------------------------------------------
class _Dataset:
    def __init__(self, n):
        self.movie_id_to_idx = {1000 + 3 * i: i for i in range(n)}


@pytest.mark.parametrize("lo,hi", [(3, 9), (20, 30)])
def test_hard_negatives_by_ppr_rank(lo, hi):
    from data.negative_sampler import NegativeSampler
    assert NegativeSampler.hard_method == "walk"
    s = NegativeSampler(_Dataset(pc.BIP_M), random_walk_sampler=_sampler("bip10"))
    assert s.hard_method == "walk"
    s.hard_method = "ppr"
    queries = [0, 5, 23, 7, 7, 11]
    q = torch.tensor(queries, device="cuda")
    np.random.seed(2024)
    out = s.sample_hard_negatives(q, num_hard_samples=4, max_rank=hi, min_rank=lo)
    state = np.random.get_state()
    fresh = np.random.RandomState(2024)
    u, u2 = fresh.random_sample((len(queries), 4)), fresh.random_sample((len(queries), 4))
    window, nwin = rw.restate(_reference_scores("bip10", tuple(queries)), pc.BIP_M, np.array(queries), lo, hi)
    picks = rw.pick(window, nwin, u, 4)
    want = rw.fill_short_rows(picks, queries, u2, pc.BIP_M)
    assert (nwin == (6 if hi == 9 else 3)).all() and ((picks < 0).any() == (hi == 30))
    assert out.dtype == torch.int64 and out.device == q.device and out.cpu().tolist() == want.tolist()
    for b, row in enumerate(out.cpu().tolist()):
        assert len(set(row)) == 4 and queries[b] not in row and all(0 <= v < pc.BIP_M for v in row)
    fs = fresh.get_state()
    assert state[0] == fs[0] and np.array_equal(state[1], fs[1]) and state[2:] == fs[2:]
    s.hard_method = "pagerank"
    with pytest.raises(ValueError, match="hard_method"):
        s.sample_hard_negatives(q)
