"""The device MT19937 generator (csrc/mt19937.hip) against np.random.RandomState, bit for bit, on the cases of
tests/helpers/mt_cases.py: every hand-back form, the state window split between two workgroups, request ends on the chunk
geometry, the scheme thresholds, every scheme at its smallest and after a skipped prefix, the base jump's high levels, and ranged
requests into a guarded buffer.  tests/test_mt_cases.py proves which planner branch / scheme / writer each case reaches.  Every
comparison is exact: doubles, raw words (numpy's tempered output untempered), all 624 state words and pos."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mt_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

N = mc.MT_N
CASES = mc.cases()
FILL32 = -1                                                 # mc.FILL as int32


def _dev():
    return torch.device("cuda")


def _run(c):
    """the case through dense.mt19937_random_sample from state_at(pos_in): (device output, state words, pos numpy is left with)"""
    from pinsage_hip import dense
    saved = np.random.get_state()
    try:
        np.random.set_state(mc.state_at(c.pos_in, c.seed).get_state())
        out = dense.mt19937_random_sample(c.n, _dev(), skip=c.skip, radix=c.radix, one_round=c.one_round, raw=c.raw,
                                          ranges=None if c.ranges is None else list(c.ranges))
        _, key, pos, _, _ = np.random.get_state()
    finally:
        np.random.set_state(saved)
    return out, key.astype(np.uint32), int(pos)


class _Stream:
    """numpy's stream from state_at(pos_in) after really skipping `skip` doubles, generated ONCE up to the longest request that
    shares it: the doubles (host, and on the device when asked for), and the state numpy is in after each of the lengths `ns`"""

    def __init__(self, pos_in, skip, ns, device=False, seed=1234):
        rs = mc.state_at(pos_in, seed)
        if skip:
            rs.random_sample(skip)
        self.skip = skip
        parts, self.state, done = [], {}, 0
        for n in sorted(set(ns)):
            parts.append(rs.random_sample(n - done))
            done = n
            _, key, pos, _, _ = rs.get_state()
            self.state[n] = (key.astype(np.uint32), int(pos))
        self.u = np.concatenate(parts)
        self.u_dev = torch.from_numpy(self.u).to(_dev()) if device else None

    def check(self, c, out, key, pos):
        off = c.skip - self.skip                           # (a case may skip further than the shared stream did)
        if self.u_dev is not None:
            assert torch.equal(out, self.u_dev[off:off + c.n]), c.name
        else:
            assert np.array_equal(out.cpu().numpy(), self.u[off:off + c.n]), c.name
        want_key, want_pos = self.state[off + c.n]
        assert pos == want_pos, (c.name, pos, want_pos)
        assert np.array_equal(key, want_key), c.name


def _raw_oracle(pos_in, nwords, seed=1234):
    """the first nwords untempered stream words from state_at(pos_in)"""
    return mc.untemper(mc.tempered_words(mc.state_at(pos_in, seed), nwords))


def test_the_library_has_the_geometry_assumed_here():
    from pinsage_hip import dense, mtjump
    from pinsage_hip import native as nv
    g = mc.GEOM
    assert nv.lib().ps_mt19937_chunk_log2() == g.chunk_log2
    assert nv.lib().ps_mt19937_window_shift() == g.window_shift
    jp, rp, wp = dense._jump_polys(_dev()), dense._radix_polys(_dev()), dense._window_polys(_dev())
    assert tuple(jp.shape) == (g.jump_levels, N) and tuple(rp.shape) == (g.radix_levels, 31, N) and tuple(wp.shape) == (g.n_window, N)
    assert (mtjump.JUMP_LEVELS, mtjump.RADIX_LEVELS, mtjump.WINDOW_POLYS) == (g.jump_levels, g.radix_levels, g.n_window)
    # the store sizes the restated room checks use (JP, SEQ_PAD) are those of the workspace the library asks for
    for K in (2, 33, 513, 1025):
        n = mc.n_for_K(K)
        p = mc.make_plan(N, 0, n)
        Kw = max(p.K + 2, 128)
        a256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
        want = a256((Kw + 4) * mc.WSZ * 4) + a256((Kw // 2 + 2) * mc.SEQ_PAD * 4) + a256((p.w_hi - p.w_lo + 2 * N + mc.CHUNK) * 4) + 4096
        assert nv.lib().ps_mt19937_workspace_bytes(0, n) == want, K


# ---- a, b, c: short requests, each against its own numpy replay -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for g in "abc" for c in mc.group(g)])
def test_short_request(name):
    """a: K = 1 on the parallel path, every hand-back form; b: the state window split between two workgroups; c: the request's
    ends on half edges, window bases and block ends.  Doubles, all 624 state words and pos."""
    c = CASES[name]
    assert mc.takes_parallel_path(c.skip, c.n)
    out, key, pos = _run(c)
    _Stream(c.pos_in, c.skip, [c.n], seed=c.seed).check(c, out, key, pos)


# ---- d: the scheme thresholds ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold_stream():
    s = _Stream(0, 0, [c.n for c in mc.group("d")], device=True)      # 67 M doubles, generated and uploaded once
    yield s
    s.u_dev = None
    torch.cuda.empty_cache()


@pytest.mark.parametrize("K", [2, 32, 33, 34, 512, 513, 1024, 1025])
def test_scheme_threshold(K, threshold_stream):
    """skip = 0, default flags, the smallest request with K chunk windows: every double (compared on the device), the state, pos"""
    c = CASES["d-K%d" % K]
    assert mc.plan_of(c).K == K
    out, key, pos = _run(c)
    threshold_stream.check(c, out, key, pos)


# ---- e: every scheme at its smallest and at a ragged K, all forms of a request against numpy and against each other ---------------------------
@pytest.fixture(scope="module")
def scheme_stream():
    e = mc.group("e")
    assert len({c.pos_in for c in e}) == 1
    s = _Stream(e[0].pos_in, 0, [c.skip + c.n for c in e], device=True)
    s.raw_dev = torch.from_numpy(_raw_oracle(e[0].pos_in, max(mc.plan_of(c).w_hi for c in e)).view(np.int32)).to(_dev())
    yield s
    s.u_dev = s.raw_dev = None


@pytest.mark.parametrize("K", [2, 3, 31, 32, 33, 45, 64, 65])
def test_every_scheme(K, scheme_stream):
    """doubling, radix (mt_combine_radix_kernel up to 32 chunks and for 33 .. 44, two MFMA rounds from 45) and the default (one round
    from 33), each as doubles and as raw words"""
    outs = {}
    for form, _ in mc.FORMS:
        for raw in ((False,) if K == 2 else (False, True)):             # (K = 2: skipped prefix, no raw form)
            c = CASES["e-K%d-%s-%s" % (K, form, "raw" if raw else "dbl")]
            p = mc.plan_of(c)
            assert p.K == K and mc.takes_parallel_path(c.skip, c.n)
            out, key, pos = _run(c)
            if raw:
                assert out.shape[0] == 2 * c.n + 2 * N and p.w_lo == 0
                out = out[:p.w_hi]
                assert torch.equal(out, scheme_stream.raw_dev[:p.w_hi]), c.name
                want_key, want_pos = scheme_stream.state[c.n]
                assert pos == want_pos and np.array_equal(key, want_key), c.name
            else:
                scheme_stream.check(c, out, key, pos)
            outs[(form, raw)] = out
    for (form, raw), out in outs.items():
        assert torch.equal(out, outs[("default", raw)]), (K, form, raw)


# ---- f: schemes after a skipped prefix ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skipped_stream():
    f = mc.group("f")
    assert len({(c.pos_in, c.skip) for c in f}) == 1
    return _Stream(f[0].pos_in, f[0].skip, [c.n for c in f], device=True)       # numpy really skips the 5 M doubles


@pytest.mark.parametrize("name", [c.name for c in mc.group("f")])
def test_scheme_after_a_skipped_prefix(name, skipped_stream):
    c = CASES[name]
    assert mc.plan_of(c).c0 == 76
    out, key, pos = _run(c)
    skipped_stream.check(c, out, key, pos)


# ---- g: the base jump's high levels -------------------------------------------------------------------------------------------------------------
def test_base_jump_high_levels():
    """skip = 4.4e12 doubles: numpy cannot go there, so the host chains mtjump.apply_jump_reference over the set bits of c0 - 1 from
    the window at stream word 1, installs that window in a RandomState and generates FORWARDS through the request -- the device
    reaches the same words through its own base jump (levels 17, 19, 30, 43) and a backward half chunk."""
    from pinsage_hip import mtjump
    c = mc.JUMP_CASE
    p = mc.plan_of(c)
    assert p.c0 == mc.JUMP_C0 and p.key_w >= 1
    window = _raw_oracle(c.pos_in, N + 1)[1:]
    for b in range(64):
        if ((p.c0 - 1) >> b) & 1:
            window = mtjump.apply_jump_reference(window, mc.GEOM.chunk_log2 + b)
    base = 1 + (p.c0 - 1) * mc.CHUNK                        # stream index of the installed window's first word
    assert base < p.w_lo
    host = np.random.RandomState(0)
    host.set_state(("MT19937", window.astype(np.uint32), 0, 0, 0.0))
    tw = mc.tempered_words(host, p.w_hi - base)
    out, key, pos = _run(c)
    assert np.array_equal(out.cpu().numpy(), mc.doubles_of(tw[p.wa - base:p.wb - base]))
    assert pos == p.pos_out and np.array_equal(key, mc.untemper(tw[p.key_w - base:p.key_w - base + N]))


def test_skip_beyond_the_jump_table_is_refused():
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    dev, n, skip = _dev(), 10, mc.BEYOND_TABLE_SKIP
    _, key, pos, _, _ = mc.state_at(3).get_state()
    st_in = torch.from_numpy(key.astype(np.uint32).view(np.int32)).to(dev)
    back = torch.full((625,), FILL32, dtype=torch.int32, device=dev)
    out = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    polys, rpolys, wpolys = dense._jump_polys(dev), dense._radix_polys(dev), dense._window_polys(dev)
    ws, wsb = nv.workspace("ps_mt19937_workspace_bytes", dev, skip, n)

    def call(s):
        with torch.cuda.device(dev):
            rc = nv.lib().ps_mt19937_random_sample(nv.ptr(st_in), int(pos), s, n, nv.ptr(out), nv.ptr(back), nv.ptr(back[624:]),
                                                   nv.ptr(polys), polys.size(0), nv.ptr(rpolys), rpolys.size(0), nv.ptr(wpolys),
                                                   wpolys.size(0), nv.ptr(ws), wsb, nv.stream())
        torch.cuda.synchronize()
        return rc
    assert call(skip) == nv.PS_EUNSUPPORTED
    assert bool((out == -1.0).all()) and bool((back == FILL32).all())              # no result, no state
    assert call(skip - mc.CHUNK) == nv.PS_OK and bool((out != -1.0).all())          # one chunk earlier the table still serves it


# ---- h: ranged requests into the interior of a larger buffer ------------------------------------------------------------------------------------------
GUARD = 1056


def _abi_raw(pos_in, n, ranges, seed=1234):
    """ps_mt19937_raw_stream through the C ABI, the buffer a view into a larger tensor pre-filled with 0xFFFFFFFF:
    (whole tensor as uint32, the 625-word hand-back)"""
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    dev = _dev()
    _, key, pos, _, _ = mc.state_at(pos_in, seed).get_state()
    st_in = torch.from_numpy(key.astype(np.uint32).view(np.int32)).to(dev)
    back = torch.full((625,), FILL32, dtype=torch.int32, device=dev)
    big = torch.full((GUARD + 2 * n + 2 * N + GUARD,), FILL32, dtype=torch.int32, device=dev)
    raw = big[GUARD:GUARD + 2 * n + 2 * N]
    polys, rpolys, wpolys = dense._jump_polys(dev), dense._radix_polys(dev), dense._window_polys(dev)
    ws, wsb = nv.workspace("ps_mt19937_workspace_bytes", dev, 0, n)
    rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
    with torch.cuda.device(dev):
        nv.call("ps_mt19937_raw_stream", nv.ptr(st_in), int(pos), n, nv.ptr(raw), nv.ptr(back), nv.ptr(back[624:]), nv.ptr(polys),
                polys.size(0), nv.ptr(rpolys), rpolys.size(0), nv.ptr(wpolys), wpolys.size(0), rg.ctypes.data, rg.shape[0],
                nv.ptr(ws), wsb, nv.stream())
    return big, back.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def ranged_oracle():
    """pos_in -> (untempered words of the whole request incl. the state window, numpy's state after n doubles)"""
    out = {}
    for pos_in in (3, 624):
        p = mc.make_plan(pos_in, 0, mc.RANGED_N)
        truth = _raw_oracle(pos_in, p.w_hi)
        assert not bool((truth == mc.FILL).any())          # the fill value does not occur in the true stream
        rs = mc.state_at(pos_in)
        rs.random_sample(mc.RANGED_N)
        _, key, pos, _, _ = rs.get_state()
        out[pos_in] = (truth, key.astype(np.uint32), int(pos))
    return out


@pytest.mark.parametrize("pos_in", [3, 624])
@pytest.mark.parametrize("name", list(mc.ranged_sets()))
def test_ranged_request(name, pos_in, ranged_oracle):
    n = mc.RANGED_N
    runs, _ = mc.ranged_sets()[name]
    truth, want_key, want_pos = ranged_oracle[pos_in]
    p = mc.make_plan(pos_in, 0, n)
    rp = mc.ranged_plan(pos_in, n, runs if len(runs) <= 3 else None)   # (four runs: the library's own planner declines them too)
    big, back = _abi_raw(pos_in, n, runs)
    big = big.cpu().numpy().view(np.uint32)
    lead, raw, trail = big[:GUARD], big[GUARD:GUARD + 2 * n + 2 * N], big[GUARD + 2 * n + 2 * N:]
    assert bool((lead == mc.FILL).all()) and bool((trail == mc.FILL).all())                    # both guard bands
    assert bool((raw[p.w_hi:] == mc.FILL).all())                                                # nothing past the state window
    must = np.zeros(p.w_hi, dtype=bool)
    must[0] = True                                                                               # word 0 always
    must[p.key_w:p.key_w + N] = True                                                             # the state's words
    if rp.ranged:
        for lo, hi in runs:
            lo, hi = max(lo, 0), min(hi, n)
            if lo < hi:
                must[2 * lo:2 * hi] = True
    else:
        must[:] = True                                                                           # whole stream
    got = raw[:p.w_hi]
    assert np.array_equal(got[must], truth[must]), name
    rest = got[~must]
    assert bool(((rest == mc.FILL) | (rest == truth[~must])).all()), name                     # unwritten or right, never else
    assert np.array_equal(back[:624], want_key) and int(back[624]) == want_pos, name


def test_four_runs_through_the_wrapper_give_the_whole_stream(ranged_oracle):
    c = CASES["h-p3-four-runs"]
    truth, want_key, want_pos = ranged_oracle[3]
    out, key, pos = _run(c)
    w_hi = mc.plan_of(c).w_hi
    assert np.array_equal(out[:w_hi].cpu().numpy().view(np.uint32), truth)
    assert pos == want_pos and np.array_equal(key, want_key)


def test_ranged_request_beyond_the_window_table():
    """514 chunks with one small run: the state window lies beyond the 511-row table, so the whole stream is generated -- and must
    be right everywhere.  Compared on the device against numpy's words, untempered there by plain integer ops."""
    c = CASES["h-table-fallback"]
    p = mc.plan_of(c)
    rs = mc.state_at(c.pos_in)
    tw = mc.tempered_words(rs, p.w_hi)
    assert not bool((tw == mc.temper(np.array([mc.FILL], dtype=np.uint32))[0]).any())          # the fill value is no true raw word
    rs = mc.state_at(c.pos_in)
    rs.random_sample(c.n)
    _, want_key, want_pos, _, _ = rs.get_state()
    truth = mc.untemper_torch(torch.from_numpy(tw.view(np.int32)).to(_dev()))
    big, back = _abi_raw(c.pos_in, c.n, list(c.ranges))
    end = GUARD + 2 * c.n + 2 * N
    assert torch.equal(big[GUARD:GUARD + p.w_hi], truth)
    assert bool((big[:GUARD] == FILL32).all()) and bool((big[end:] == FILL32).all()) and bool((big[GUARD + p.w_hi:end] == FILL32).all())
    assert np.array_equal(back[:624], want_key.astype(np.uint32)) and int(back[624]) == int(want_pos)
