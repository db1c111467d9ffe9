"""The device MT19937 generator's case table (tests/helpers/mt_cases.py) proves its own coverage here, without a GPU: which
hand-back form, which split of the state window, which scheme, which window runs every case reaches follows from the restated
planners, and is asserted before tests/test_hip_mt_stream.py runs the kernels on the cases.  The restated plan is held to numpy
(the state it predicts IS RandomState.get_state()), the oracles to each other, and every perturbation of the restatement must be
noticed by a named case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mt_cases as mc  # noqa: E402

N, CHUNK, HALF = mc.MT_N, mc.CHUNK, mc.HALF
CASES = mc.cases()


def _props(c):
    p, rp, ws = mc.writers_of(c)
    return p, rp, ws, mc.scheme_of(c)


def test_the_thresholds_come_out_of_the_bisection():
    got = [mc.n_for_K(K) for K in (2, 32, 33, 512, 513, 1024, 1025)]
    assert got == [32761, 1998673, 2064193, 33456073, 33521593, 67010425, 67075945]
    for K, n in zip((2, 32, 33, 512, 513, 1024, 1025), got):
        assert mc.make_plan(0, 0, n).K == K and mc.make_plan(0, 0, n - 1).K == K - 1
    # which code makes the windows either side of each threshold, default flags and with one flag off
    assert [mc.scheme(K) for K in (1, 2, 32, 33, 34, 512, 513, 1024, 1025)] == \
        ["none", "combine1", "combine1", "one_round", "one_round", "one_round", "two_round", "two_round", "combine3"]
    assert [mc.scheme(K, radix=False) for K in (2, 3, 32, 33)] == ["doubling"] * 4
    # one_round=False: the parity planes of two MFMA rounds need the room of 44 stored windows, so 33 .. 44 chunks take two levels
    # of mt_combine_radix_kernel (reached by nothing else below 1025 chunks) and 45 is the smallest two-round request
    assert [mc.scheme(K, one_round=False) for K in (2, 31, 32, 33, 44, 45, 64, 65, 1024)] == \
        ["combine1", "combine1", "combine1", "combine2", "combine2", "two_round", "two_round", "two_round", "two_round"]
    assert [(K - 1) // 32 for K in (45, 64, 65)] == [1, 1, 2]                  # JA 1 -> 2
    assert mc.scheme(33, c0=76) == "one_round_fold" and mc.scheme(45, c0=76, one_round=False) == "two_round"


def test_oracle_identities():
    # randint(0, 2^32, uint32) is the word stream, two words per double, from every block position
    for pos_in in mc.POS_EDGES + (5, 311):
        w = mc.tempered_words(mc.state_at(pos_in), 4000)
        assert np.array_equal(mc.doubles_of(w), mc.state_at(pos_in).random_sample(2000))
        # raw word 0 is the state word the generator stands on
        if pos_in < N:
            assert int(mc.untemper(w[:1])[0]) == int(mc.state_at(pos_in).get_state()[1][pos_in])
    # tempering is a bijection and untemper its inverse, on the corners and on a stream
    x = np.concatenate([np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0x9d2c5680, 0xefc60000], dtype=np.uint32),
                        mc.tempered_words(np.random.RandomState(9), 200000)])
    assert np.array_equal(mc.temper(mc.untemper(x)), x) and np.array_equal(mc.untemper(mc.temper(x)), x)
    import torch
    t = mc.untemper_torch(torch.from_numpy(x.view(np.int32)))
    assert t.dtype == torch.int32 and np.array_equal(t.numpy().view(np.uint32), mc.untemper(x))


_words = {}


def _raw_stream(pos_in, m):
    """the first m untempered stream words from state_at(pos_in), cached at the longest length asked for"""
    if pos_in not in _words or _words[pos_in].shape[0] < m:
        _words[pos_in] = mc.untemper(mc.tempered_words(mc.state_at(pos_in), m))
    return _words[pos_in]


def _numpy_state(c):
    rs = mc.state_at(c.pos_in, c.seed)
    rs.random_sample(c.skip + c.n)
    _, key, pos, _, _ = rs.get_state()
    return key.astype(np.uint32), int(pos)


SMALL = [c for c in CASES.values() if c.skip + c.n <= 6_000_000]


def test_the_restated_plan_predicts_numpys_state():
    """key_w / pos_out of the restated make_plan against RandomState.get_state(), for every case short enough to replay here"""
    assert {c.name[0] for c in SMALL} >= set("abch") and len(SMALL) > 150
    longest = {}
    for c in SMALL:
        longest[c.pos_in] = max(longest.get(c.pos_in, 0), mc.plan_of(c).w_hi)
    for c in SMALL:
        p = mc.plan_of(c)
        key, pos = _numpy_state(c)
        assert pos == p.pos_out, c.name
        if p.key_w >= 0:
            got, _ = mc.state_from_words(p, _raw_stream(c.pos_in, longest[c.pos_in]))
            # (the first word of a never-regenerated block keeps only its top bit in the recurrence, but get_state returns it whole)
            assert np.array_equal(got, key), c.name
        else:
            assert np.array_equal(key, mc.state_at(c.pos_in, c.seed).get_state()[1]), c.name
        assert p.w_lo <= p.wa and p.w_hi >= p.wb and (p.key_w < 0 or (p.w_lo <= p.key_w and p.key_w + N <= p.w_hi)), c.name


def test_every_wanted_word_has_exactly_one_writer():
    for c in list(CASES.values()) + [mc.JUMP_CASE]:
        p, rp, ws, _ = _props(c)
        wanted = rp.words if rp is not None else [(p.w_lo, p.w_hi)]
        assert mc.stored_runs(ws, wanted) == mc.wanted_runs(wanted), c.name
        for a, b in zip(ws, ws[1:]):
            assert a.hi <= b.lo, c.name                    # the hulls are disjoint
        if p.key_w >= 1:
            assert 1 <= len(mc.state_writers(p, ws)) <= 2, c.name


def _some(group, pred):
    return [c.name for c in mc.group(group) if pred(*_props(c))]


def test_a_hand_back_forms():
    a = mc.group("a")
    assert {(c.pos_in, c.n) for c in a} >= {(pos, n) for pos in mc.POS_EDGES for n in (1, 2, 311, 312, 313)}
    for c in a:
        p, _, ws, sch = _props(c)
        assert p.K == 1 and p.c0 == 0 and sch == "none" and c.skip > 0 and mc.takes_parallel_path(c.skip, c.n), c.name
    assert _some("a", lambda p, rp, ws, s: p.key_w < 0)
    assert "a-p0-s1-n1" in _some("a", lambda p, rp, ws, s: p.key_w == 0)                       # mt_final_state_kernel
    assert "a-p5-s1-n1" in _some("a", lambda p, rp, ws, s: p.key_w < 0)                        # the state copy, pos moves
    assert "a-p0-s311-n1" in _some("a", lambda p, rp, ws, s: p.pos_out == N and p.key_w == 0)  # r == 0 folded to 624
    assert _some("a", lambda p, rp, ws, s: p.key_w == 1)
    assert _some("a", lambda p, rp, ws, s: p.key_w >= N)
    assert _some("a", lambda p, rp, ws, s: p.pos_out == N and p.key_w >= N)
    assert mc.plan_of(CASES["a-p624-s1-n1"]).key_w == 0                                        # ... and from a spent block
    assert {mc.key_class(mc.plan_of(c)) for c in a} == {"copy", "final_state_kernel", "chunk_kernel"}


def test_b_state_window_split_between_two_workgroups():
    p = mc.plan_of(CASES["b-half-issue"])
    assert (p.key_w, p.w_hi, p.K) == (65520, 66144, 2)
    for c in mc.group("b"):
        p, _, ws, sch = _props(c)
        want = "half" if "-half" in c.name else "base"
        assert mc.straddle(p, ws) == want and c.n == 1, c.name
        assert (p.K, sch) == ((2, "doubling" if not c.radix else "combine1") if want == "half" else (1, "none")), c.name
        assert p.c0 == (77 if "-c77" in c.name else 79 if "-c79" in c.name else 0 if want == "half" else 1), c.name
    for tag in ("b-half-p", "b-base-p", "b-half-c77", "b-base-c79"):
        sub = [mc.plan_of(c) for c in mc.group("b") if c.name.startswith(tag)]
        assert any(p.w_lo < p.wa for p in sub) and any(p.w_hi > p.wb for p in sub) and any(p.w_lo == p.wa for p in sub), tag
    # after the base jump the two writers of the half-edge cases are slots q and q + 1
    p, _, ws, _ = _props(CASES["b-half-c77-p623-hi-default"])
    assert [(w.window - p.c0, w.back) for w in mc.state_writers(p, ws)] == [(0, False), (1, True)] and p.c0 == 77


def test_c_request_ends_against_the_chunk_geometry():
    for tag, edge in (("half", 1 + CHUNK + HALF), ("base", 1 + 2 * CHUNK)):
        for d in (-1, 0, 1):
            s, e = CASES["c-start-%s%+d" % (tag, d)], CASES["c-end-%s%+d" % (tag, d)]
            assert 2 * s.skip == edge - 1 + 2 * d and 2 * (e.skip + e.n) == edge - 1 + 2 * d
            assert mc.plan_of(s).K >= 2 and mc.plan_of(e).K >= 2
        # the uniform at d = 0 has one word either side of the edge
        assert 2 * CASES["c-start-%s+0" % tag].skip < edge <= 2 * CASES["c-start-%s+0" % tag].skip + 1
    for res in (N - 1, 0, 1):
        blocks = set()
        for extra in (0, 312):
            p, _, ws, _ = _props(CASES["c-fwd-end-r%d-x%d" % (res, extra)])
            w = ws[-1]
            assert not w.back and w.hi == p.w_hi and (w.hi - w.wbase) % N == res
            blocks.add(((w.hi - w.wbase + N - 1) // N) % 2)
            p, _, ws, _ = _props(CASES["c-bwd-start-r%d-x%d" % (res, extra)])
            w = ws[0]
            assert w.back and w.lo == p.w_lo and (w.wbase - w.lo) % N == res
            blocks.add(2 + ((w.wbase - w.lo + N - 1) // N) % 2)
        assert blocks == {0, 1, 2, 3}, res                  # both parities of the chains' two-block unrolling
    # the kept words end with the last word of a forward half chunk / with the first (farthest) word of a backward one
    p, _, ws, _ = _props(CASES["c-whi-fwd-last"])
    assert p.w_hi == 1 + 2 * CHUNK + HALF and (ws[-1].window, ws[-1].back, ws[-1].hi) == (2, False, p.w_hi) and p.K == 3
    p, _, ws, _ = _props(CASES["c-whi-back-first"])
    assert p.w_hi == 2 + 2 * CHUNK + HALF and (ws[-1].window, ws[-1].back, ws[-1].hi - ws[-1].lo) == (3, True, 1) and p.K == 4


def test_d_e_f_schemes():
    want = {2: "combine1", 32: "combine1", 33: "one_round", 34: "one_round", 512: "one_round", 513: "two_round", 1024: "two_round",
            1025: "combine3"}
    for K, sch in want.items():
        c = CASES["d-K%d" % K]
        assert (mc.plan_of(c).K, mc.scheme_of(c)) == (K, sch) and (c.pos_in, c.skip, c.radix, c.one_round) == (0, 0, True, True)
    assert (34 - 1 + 31) // 32 == 2 and (34 - 1) - 32 == 1                   # K = 34: the second polynomial group is one row deep
    reach = {}
    for c in mc.group("e"):
        p = mc.plan_of(c)
        assert p.c0 == 0 and c.pos_in % 2 == 1 and (c.skip > 0) == (p.K == 2)
        reach.setdefault(mc.scheme_of(c), set()).add((p.K, c.raw))
    for sch, Ks in (("doubling", (2, 3, 32, 33)), ("combine1", (2, 31, 32)), ("combine2", (33,)), ("two_round", (45, 64, 65)),
                    ("one_round", (33,))):
        for K in Ks:
            assert {(K, False), (K, True)} - reach[sch] <= {(2, True)}, (sch, K)      # (no raw form below 2^17 doubles)
    f = {c.name: (mc.plan_of(c), mc.scheme_of(c)) for c in mc.group("f")}
    assert {s for _, s in f.values()} == {"doubling", "combine1", "combine2", "two_round", "one_round_fold"}
    for name, (p, sch) in f.items():
        assert p.c0 == 76 and CASES[name].skip > 5_000_000 and CASES[name].pos_in % 2 == 1
        assert p.K == {"doubling": 33, "combine1": 32, "combine2": 33, "two_round": 45, "one_round_fold": 33}[sch]


def test_which_cases_take_the_parallel_path():
    """skip > 0 or n >= 2^17.  From the stream's start that is K >= 3: the issue's threshold case K = 2 (n = 32761, skip = 0) runs
    the serial kernel and is kept as such; K = 2 on the parallel path is b's and e's (skipped prefix)."""
    serial = [c.name for c in CASES.values() if not mc.takes_parallel_path(c.skip, c.n)]
    assert serial == ["d-K2"]
    assert mc.make_plan(0, 0, 1 << 17).K == 3 and mc.make_plan(N, 0, 1 << 17).K == 3
    assert all(c.skip == 0 and c.n >= (1 << 17) for c in CASES.values() if c.raw)


def test_g_base_jump_levels():
    c = mc.JUMP_CASE
    p, _, ws, sch = _props(c)
    assert p.c0 == mc.JUMP_C0 and p.K == 2 and sch == "combine1"
    levels = [mc.GEOM.chunk_log2 + b for b in range(64) if (p.c0 >> b) & 1]
    assert max(levels) == 43 and sum(l >= 24 for l in levels) >= 2 and max(levels) < mc.GEOM.jump_levels
    assert ws[0].back and ws[0].lo == p.wa                  # the request opens in a backward half chunk
    assert (p.c1 >> (mc.GEOM.jump_levels - mc.GEOM.chunk_log2)) == 0
    q = mc.make_plan(0, mc.BEYOND_TABLE_SKIP, 10)
    assert (q.c1 >> (mc.GEOM.jump_levels - mc.GEOM.chunk_log2)) == 1


def test_h_ranged_requests():
    sets = mc.ranged_sets()
    for pos_in in (3, 624):
        rp = {name: mc.ranged_plan(pos_in, mc.RANGED_N, runs) for name, (runs, _) in sets.items()}
        p = mc.make_plan(pos_in, 0, mc.RANGED_N)
        assert p.K == 42 and p.key_w > 0
        key = (p.key_w, p.key_w + N)
        assert all(r.ranged for name, r in rp.items() if name != "four-runs")
        assert len(rp["four-window-runs"].wins) == 4 and rp["four-window-runs"].wins[0][0] > 1 and rp["four-window-runs"].Kw == 5
        assert rp["across-half-edge"].wins[0] == (7, 8) and rp["across-half-edge"].words[0][1] - rp["across-half-edge"].words[0][0] == 2
        assert rp["before-half-edge"].wins[0] == (7, 7) and rp["after-half-edge"].wins[0] == (8, 8)
        a, b = rp["across-window-base"].words[0]
        assert (a, b) == (9 * CHUNK, 9 * CHUNK + 2) and rp["across-window-base"].wins[0] == (9, 9)
        ws = mc.writers(p, mc.window_list(p, rp["across-window-base"]), rp["across-window-base"].words)
        assert [(w.window, w.back, w.hi - w.lo) for w in ws[:2]] == [(9, True, 1), (9, False, 1)]
        assert rp["adjacent-windows"].wins[0] == (5, 6) and len(rp["adjacent-windows"].words) == 3
        assert rp["touching-overlapping"].words == [(200, 800), key]
        assert rp["into-key-window"].words == [(2 * (mc.RANGED_N - 100), key[1])]
        assert rp["clamped-and-empty"].words == [(0, 20), (min(key[0], 2 * (mc.RANGED_N - 3)), key[1])]
        # a block of which exactly one word is wanted: forward and backward blocks of window 12
        wb = 1 + 12 * CHUNK
        (a0, _), (a1, _) = rp["block-last-word"].words[:2]
        assert (wb - a0) % N == 1 and a0 < wb and (a1 - wb) % N == N - 1 and a1 > wb
        (_, b0), (_, b1) = rp["block-first-word"].words[:2]
        assert (wb - (b0 - 1)) % N == 0 and b0 < wb and (b1 - 1 - wb) % N == 0 and b1 > wb
        assert rp["everything"].words == [(0, p.w_hi)] and rp["everything"].Kw == p.K
        assert not rp["four-runs"].ranged and rp["four-runs"].why == "more than three runs"
    c = CASES["h-table-fallback"]
    r = mc.ranged_plan(c.pos_in, c.n, c.ranges)
    assert not r.ranged and r.why == "beyond the window table" and mc.plan_of(c).K == 515
    assert mc.ranged_plan(3, 510 * HALF, c.ranges).ranged      # (one chunk run below the table's end it is still ranged)


def _windows_and_words(c, **kw):
    """what a (perturbed) restatement expects: plan, window slots, and the words that get a writer"""
    pkw = {k: v for k, v in kw.items() if k in ("fold_r0", "extend_hi", "half_shift")}
    p = mc.plan_of(c, **pkw)
    if c.raw and c.ranges is not None:
        rkw = {k: v for k, v in kw.items() if k != "fold_r0"}
        rp = mc.ranged_plan(c.pos_in, c.n, c.ranges, **rkw)
        wanted = rp.words
    else:
        rp, wanted = None, [(p.w_lo, p.w_hi)]
    wins = mc.window_list(p, rp)
    return p, wins, wanted, mc.stored_runs(mc.writers(p, wins, wanted), wanted)


TEETH = [
    # perturbation, the case that must notice, what changes
    (dict(half_shift=1), "h-p3-across-half-edge", "windows"),       # the half edge one word later: window 7 is not launched
    (dict(half_shift=-1), "h-p3-across-half-edge", "windows"),      # one word earlier: window 8 is not launched
    (dict(half_shift=1), "c-start-half+0", "windows"),              # whole stream: the request's first word is a half chunk's last
    (dict(half_shift=-1), "c-whi-back-first", "windows"),           # ... its last kept word a half chunk's first
    (dict(drop_key=True), "h-p3-across-half-edge", "wanted"),
    (dict(chi_from_b=True), "h-p3-before-half-edge", "windows"),
    (dict(fold_r0=False), "a-p0-s311-n1", "state"),
    (dict(extend_hi=False), "b-half-p0-lo-default", "windows"),
]


@pytest.mark.parametrize("kw,name,what", TEETH, ids=["%s:%s" % (sorted(k)[0], n) for k, n, _ in TEETH])
def test_teeth(kw, name, what):
    """every perturbation of the restatement changes what a named table case expects, so the device run of that case (which is
    held to numpy word for word) would notice the same slip in the kernel's planner"""
    c = CASES[name]
    p0, wins0, wanted0, stored0 = _windows_and_words(c)
    p1, wins1, wanted1, stored1 = _windows_and_words(c, **kw)
    assert stored0 == mc.wanted_runs(wanted0)
    if what == "windows":
        assert wins1 != wins0 or p1.K != p0.K
        # and with the perturbed window set, words the case checks have no writer, or a workgroup is launched for nothing
        assert stored1 != mc.wanted_runs(wanted0) or len(wins1) > len(wins0)
    elif what == "wanted":
        assert mc.wanted_runs(wanted1) != mc.wanted_runs(wanted0)
        assert not any(a <= p0.key_w and p0.key_w + N <= b for a, b in stored1)    # the state's words are never produced
    else:
        key, pos = _numpy_state(c)
        assert (p0.pos_out, p0.key_w) != (p1.pos_out, p1.key_w) and p0.pos_out == pos == N and p1.pos_out == 0


def test_a_ranged_request_always_takes_a_product():
    """mt_generate's branch "a ranged request inside window 0's half chunk" (no product, nprod == 0) cannot be reached through
    ps_mt19937_raw_stream: it refuses n < 2^17, and the state's 624 words -- always wanted -- then end beyond window 0's half chunk"""
    def nprod(pos_in, n, runs):
        r = mc.ranged_plan(pos_in, n, runs)
        return r.Kw - 1 if r.ranged else None
    for c in mc.group("h"):
        assert nprod(c.pos_in, c.n, c.ranges) != 0, c.name
    for pos_in in tuple(range(0, N + 1, 13)) + mc.POS_EDGES:
        for n in sorted(set([1 << 17, (1 << 17) + 1, (1 << 17) + 311, (1 << 17) + 312, 3 * HALF, 200000, 41 * HALF, 510 * HALF])):
            p = mc.make_plan(pos_in, 0, n)
            assert p.key_w + N - 1 >= 1 + HALF             # the state's last word lies in window >= 1
            for runs in ([(0, 1)], [(5, 6), (n - 1, n)], [(0, n)], [(100, 50)]):
                k = nprod(pos_in, n, runs)
                assert k is not None and k >= 1, (pos_in, n, runs)
    # below the entry point's limit the branch is real: the restatement reaches it
    assert nprod(0, 1000, [(0, 10)]) == 0 and mc.scheme(1, ranged=True, Kw=1) == "one_round_empty"
