"""The fused GCN layer's and the pooling's case table (tests/helpers/gcn_cases.py) proves itself here, without a GPU: by the
restated launcher every case produces the situation it names (the planted counts of heavy rows, the tile that mixes both classes,
two passes per chunk, the partial last chunk, second pooling sweeps, kmax from each lane group, every kind of row metadata), the
exact pooling oracle (oracle.c_oracle.pool_ex) stays inside the bound derived in the helper around an fp64 restatement of
ImportancePooling.forward on every pooling case, its two summation orders agree bit for bit at T <= 16, and it agrees with the
older orc_importance_pool where both can express the case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gcn_cases as gn  # noqa: E402
import gemm_cases as gc  # noqa: E402

BY_NAME = {c.name: c for c in gn.FUSED_CASES + gn.UNSERVED_CASES}


def test_the_launcher_restated():
    assert [gn.gcn_chunk_rows(M) for M in (1, 24576, 1024 * 256, 1024 * 256 + 1, gn.BIG_M, 1024 * 512 + 1)] == \
        [256, 256, 256, 512, 512, 768]
    ok = dict(M=gn.MANY_ROWS, K=32, N=256, H=64, T=16)
    assert gn.gcn_served(**ok)
    for change in (dict(M=gn.MANY_ROWS - 1), dict(T=17), dict(N=128), dict(K=36), dict(H=68), dict(relu=False), dict(l2=False),
                   dict(env=(("PS_GCN_FUSED", "0"),)), dict(env=(("PS_POOL_ROWS_PER_WAVE", "1"),)), dict(env=(("PS_GEMM_SHARD", "2"),)),
                   dict(w_first=1, ldw=36), dict(ldw2=66)):
        assert not gn.gcn_served(**{**ok, **change}), change
    assert gn.gcn_served(**{**ok, **dict(env=(("PS_GCN_FUSED", "1"),), w2_first=32, ldw=96, ldw2=96)})
    keeps = np.array([0, 1, 1, 0, 0, 1], dtype=bool)
    ord_, nheavy = gn.partition(keeps)
    assert ord_.tolist() == [1, 2, 5, 0, 3, 4] and nheavy == 3
    ids = np.array([[5, -1], [9, 2], [-1, 3], [3, 3]], dtype=np.int32)
    assert gn.row_keeps(ids, np.array([1, 1, 1, 0], dtype=np.int32), 2, 8).tolist() == [True, False, False, False]
    assert gn.row_keeps(ids, np.array([7, 7, 2, -1], dtype=np.int32), 2, 8).tolist() == [True, True, True, False]


def test_the_table_is_the_issue_s():
    names = [c.name for c in gn.FUSED_CASES + gn.UNSERVED_CASES]
    assert len(set(names)) == len(names)
    fused = gn.FUSED_CASES
    assert {(c.K, c.H) for c in fused} >= {(256, 256), (128, 256), (32, 64), (64, 288), (32, 512)}
    assert {c.M for c in fused} == {gn.MANY_ROWS, gn.RAGGED, gn.BIG_M} and gn.RAGGED == 64 * 384 + 37
    assert {c.T for c in fused} >= {1, 4, 5, 16}
    assert {(c.form, r) for c in fused for r in c.renorms} == {("counts", 0), ("counts", 1), ("wts", 0), ("wts", 1)}
    assert {c.pattern for c in fused} == {"none", "last_only", "64j", "64j+1", "all_but_row0", "all", "mixed", "two_pass"}
    assert any(c.h_is_x for c in fused) and any(not c.h_is_x and c.extra > 0 for c in fused)
    assert sum(c.wslice for c in fused) == 1 and any(c.max_idx_above for c in fused)
    for c in fused:
        first2, ld = (c.K, c.K + c.H) if c.wslice else (0, None)
        assert c.served and gn.gcn_served(c.M, c.K, 256, c.H, c.T, w2_first=first2, ldw=ld, ldw2=ld), c.name
    for c in gn.UNSERVED_CASES:
        assert not c.served and not gn.gcn_served(c.M, c.K, 256, c.H, c.T), c.name
    assert {(c.M < gn.MANY_ROWS, c.T) for c in gn.UNSERVED_CASES} == {(True, 10), (False, 17), (False, 50)}
    off = BY_NAME[gn.SWITCHED_OFF_CASE]
    assert off.served and not gn.gcn_served(off.M, off.K, 256, off.H, off.T, env=(("PS_GCN_FUSED", "0"),))
    # pooling cases
    four = [c for c in gn.POOL_CASES if c.kernel == "four"]
    wave = [c for c in gn.POOL_CASES if c.kernel == "wave"]
    assert {c.T for c in four} == {1, 16, 17, 33, 64} and {c.T for c in wave} == {10, 16, 64, 65, 100}
    assert {c.H for c in gn.POOL_CASES} == {4, 7, 32, 256, 260, 512}
    for c in gn.POOL_CASES:
        assert gn.pool_kernel(c.T, c.H, c.env) == c.kernel and c.B % 4 != 0 and c.B > 16, c.name
    assert any(c.H % 4 for c in wave) and any(c.T > 64 and not c.env for c in wave) and any(c.T <= 64 and c.env for c in wave)


EXPECT = {                                # name -> what facts() must say
    "k256h256-T16-mixed-counts-hx": dict(last_tile_heavy=False, last_tile_rows=37, kmax_groups=[0, 1, 2, 3], sweeps=1),
    "k128h256-T5-mixed-wts": dict(last_tile_rows=64, kmax_groups=[0, 1, 2, 3]),
    "k32h64-T1-none-counts": dict(nheavy=0, mixed_tile=None),
    "k32h64-T4-last-only-counts": dict(nheavy=1, mixed_tile=0, last_tile_heavy=False),
    "k32h64-T4-64j-wts": dict(nheavy=64 * 191, mixed_tile=None, kmax_groups=[0, 1, 2, 3]),
    "k32h64-T5-64j+1-counts": dict(nheavy=64 * 191 + 1, mixed_tile=191, kmax_groups=[0, 1, 2, 3]),
    "k32h64-T16-all-but-row0-counts": dict(nheavy=gn.MANY_ROWS - 1, mixed_tile=383, last_tile_heavy=True),
    "k32h64-T4-all-wts": dict(nheavy=gn.RAGGED, mixed_tile=None, last_tile_heavy=True, last_tile_rows=37),
    "k64h288-T5-mixed-counts": dict(sweeps=2, last_sweep_cols=32, last_tile_heavy=False, last_tile_rows=37),
    "k32h512-T4-mixed-wts": dict(sweeps=2, last_sweep_cols=256),
    "k32h64-T4-mixed-counts-slices-above": dict(chunk=256, passes=1),
    "k32h32-T2-two-pass-counts": dict(chunk=512, passes=2, nchunks=513),
}


@pytest.mark.parametrize("c", gn.FUSED_CASES + gn.UNSERVED_CASES, ids=lambda c: c.name)
def test_case_produces_its_situation(c):
    d = gn.gcn_data(c)
    f = gn.facts(c)
    M, T = c.M, c.T
    rows = d.rows
    ord_, nheavy = gn.partition(d.keeps)
    assert np.array_equal(gn.row_keeps(rows.ids, rows.nvalid, T, min(d.max_idx_arg, d.n_full - 1)), d.keeps)
    assert np.array_equal(np.sort(ord_), np.arange(M)) and bool(d.keeps[ord_[:nheavy]].all()) and not d.keeps[ord_[nheavy:]].any()
    assert bool((np.diff(ord_[:nheavy]) > 0).all()) and bool((np.diff(ord_[nheavy:]) > 0).all())
    if c.served:
        for key, want in EXPECT[c.name].items():
            assert f[key] == want, (c.name, key, f[key], want)
    # the pattern's own promise
    if c.pattern == "last_only":
        assert np.flatnonzero(d.keeps).tolist() == [M - 1]
    if c.pattern == "all_but_row0":
        assert np.flatnonzero(~d.keeps).tolist() == [0] and ord_[-1] == 0
    if c.pattern == "mixed":
        assert f["mixed_tile"] is not None and 0 < f["mixed_tile"] < f["ntiles"] - 1
        assert len(d.planted) == min(3, 64 - nheavy % 64) and all(not d.keeps[i] for i in d.planted)
        pos = {int(i): p for p, i in enumerate(ord_)}
        for i in d.planted:                                                # an empty row of the tile that pools: x row of -0.0
            assert pos[i] // 64 == f["mixed_tile"] and bool(np.signbit(d.x[i]).all()) and not d.x[i].any()
        assert d.b[0] == 0.0
    if c.pattern == "two_pass":
        chunk = f["chunk"]
        assert M == 1024 * 256 + 256 + 5 and chunk == 512 and f["passes"] == 2
        last = M - (f["nchunks"] - 1) * chunk
        assert 256 < last < chunk                                          # the last chunk is partial and still takes two passes
        kp = np.zeros(f["nchunks"] * chunk, dtype=bool)
        kp[:M] = d.keeps
        inm = np.arange(kp.size) < M
        h = (kp & inm).reshape(-1, 2, 256).sum(axis=2)                     # heavy rows per (chunk, pass)
        e = (~kp & inm).reshape(-1, 2, 256).sum(axis=2)
        assert bool(((h[:, 0] > 0) & (h[:, 1] > 0) & (e[:, 0] > 0) & (e[:, 1] > 0)).any())      # both classes in both passes
        assert bool(((h[:, 0] == 0) & (h[:, 1] == 256)).any())             # a heavy second pass after an empty first
        assert bool(((h[:, 0] == 256) & (h[:, 1] == 0)).any())
        assert h[-1, 1] + e[-1, 1] == last - 256 == 5
    # row metadata: every kind the table promises is present, in ordinary surroundings
    k = np.clip(rows.nvalid, 0, T)
    inside = np.arange(T)[None, :] < k[:, None]
    keep = inside & (rows.ids >= 0) & (rows.ids <= d.max_idx)
    heavy_any = nheavy >= 16
    if heavy_any:
        assert bool((rows.nvalid[d.keeps] > T).any()) and bool((rows.nvalid == 2 ** 31 - 1).any())
        assert bool((keep & (rows.ids == d.max_idx)).any())                                        # a kept id == max_idx
        if T > 1:
            assert bool((inside & (rows.ids == -1))[d.keeps].any())                                # -1 pads inside j < k
            assert bool((inside & (rows.ids > d.max_idx))[d.keeps].any())                          # too large, still in tot
            assert bool((keep.sum(axis=1) == 1)[rows.kind == gn.LAST_SLOT_ONLY].all()) and bool(keep[rows.kind == gn.LAST_SLOT_ONLY, T - 1].all())
        if c.form == "counts" and T > 1:
            assert bool((keep & (rows.counts == 0)).any())                                         # a kept count of 0, tot > 0
            assert bool(((inside & (rows.ids > d.max_idx)) * rows.counts).any())
        if c.form == "wts":
            w = np.where(keep, rows.wts, np.float32(0)).astype(np.float64)
            s = w.sum(axis=1)
            assert bool((s[rows.kind == gn.ZERO_SUM] == 0).all()) and bool((rows.kind == gn.ZERO_SUM).any())
            assert bool((s[rows.kind == gn.NEG_SUM] < 0).all()) and bool((rows.kind == gn.NEG_SUM).any())
            assert bool(d.keeps[np.isin(rows.kind, (gn.ZERO_SUM, gn.NEG_SUM))].all())
            assert bool((w[s > 0] >= 0).all())                                                     # what is divided is non-negative
    if nheavy <= M - 16:
        em = ~d.keeps
        assert bool(((rows.nvalid == 0) & em & ((rows.ids >= 0) & (rows.ids <= d.max_idx)).any(axis=1)).any())   # nvalid = 0 over valid ids
        assert bool((rows.nvalid[em] > 0).any()) and bool((rows.nvalid[em] < 0).any())
    if c.form == "counts":
        assert bool(((rows.counts * inside).sum(axis=1)[k > 0] > 0).all())                         # no row has tot == 0
    assert c.max_idx_above == (d.max_idx_arg > d.n_full - 1) and d.max_idx == min(d.max_idx_arg, d.n_full - 1)
    assert bool((rows.ids >= d.n_full).any()) and rows.ids.max() < d.n_full + 9 and rows.ids.min() == -1
    # ordinary numbers wherever a wrong index would land
    assert d.n_full >= M and bool(d.h_full[d.max_idx + 1:].all()) and bool(d.Wbig.all())
    assert (d.h_full is d.x) == c.h_is_x and d.h_full.shape == (d.n_full, c.H) and (c.h_is_x or d.n_full > M)
    assert np.array_equal(d.Wbig[:, :c.K], d.W) and np.array_equal(d.Wbig[:, c.K:], d.W2)
    if T > 1:
        beyond = (~inside) & (rows.ids >= 0) & (rows.ids <= d.max_idx)
        assert bool(beyond.any())                                                                  # valid ids beyond nvalid


def test_only_the_two_pass_case_sees_a_lost_carry():
    """The order kernel restated pass by pass gives the stable partition on every case; with hoff not carried from one pass to
    the next it still does wherever a chunk is one pass, and leaves slots of the order unwritten in the two-pass case: rows of y
    that stay NaN."""
    for c in gn.FUSED_CASES:
        keeps = gn.gcn_data(c).keeps
        ord_, nheavy = gn.partition(keeps)
        got, total = gn.order_by_passes(keeps)
        assert total == nheavy and np.array_equal(got, ord_), c.name
        lost, _ = gn.order_by_passes(keeps, carry=False)
        assert np.array_equal(lost, ord_) == (c.pattern != "two_pass"), c.name
        if c.pattern == "two_pass":
            assert int((lost < 0).sum()) > 1000


@pytest.mark.parametrize("c", [c for c in gn.FUSED_CASES if c.M < gn.BIG_M], ids=lambda c: c.name)
def test_fused_reference_is_what_the_case_needs(c):
    """The oracle's output of a fused case: finite, rows that keep nothing pooled to +0 bits and the others not, the planted
    -0.0 rows reduced to the bias, and -- the reason the fused kernel may skip W2 -- the oracle's own normalised output inside
    norm_bound(256) of the fp64 norm."""
    from oracle import c_oracle as co
    d = gn.gcn_data(c)
    for renorm in c.renorms:
        pooled, pre = gn.gcn_ref(c, renorm)
        assert pooled.shape == (c.M, c.H) and pre.shape == (c.M, 256) and bool(np.isfinite(pre).all())
        assert not pooled[~d.keeps].view(np.uint32).any()
        ordinary = d.keeps & np.isin(d.rows.kind, (gn.ORDINARY, gn.NV_ABOVE_T, gn.AT_MAX_IDX, gn.NV_FULL, gn.LAST_SLOT_ONLY))
        if c.form == "wts" or c.T == 1:
            assert bool(pooled[ordinary].any(axis=1).all())
        for i in d.planted:
            assert np.array_equal(pre[i], np.maximum(d.b, 0)) and not pre[i, :1].view(np.uint32).any()
        if renorm != c.renorms[0]:
            continue                                                       # the norm's bound once per case: it does not depend on renorm
        got = co.linear(d.x, d.W, d.b, x2=pooled, W2=d.W2, relu=True, l2norm=True, threads=8)
        assert not gn.gcn_mismatches(got, c, renorm)
        broken = got.copy()
        broken[-1, -1] = np.nan                                            # a row the kernel never wrote
        assert [m[:2] for m in gn.gcn_mismatches(broken, c, renorm)] == [(c.M - 1, 255)]


def _pool64(c, form, renorm):
    d = gn.pool_data(c)
    counts, wts = gn.form_args(d.rows, form)
    return gn.ref_pool64(d.x, d.rows.ids, counts, wts, d.rows.nvalid, d.max_idx, renorm)


@pytest.mark.parametrize("c", gn.POOL_CASES, ids=lambda c: c.name)
def test_pool_oracle_meets_its_derived_bound(c):
    d = gn.pool_data(c)
    rows, T = d.rows, c.T
    assert rows.nvalid[-1] > T and d.keeps[-1]                             # the last row: its excess would be beyond the buffers
    assert bool((rows.nvalid > T).sum() >= 2) and bool((rows.nvalid == 0).any()) and bool((rows.nvalid < 0).any())
    assert rows.ids.max() > c.N - 1 and rows.ids.min() == -1 and bool((rows.ids == d.max_idx).any())
    for form, renorm in gn.POOL_RUNS:
        ref, S, div, nonneg = _pool64(c, form, renorm)
        assert bool(nonneg[div].all())                                     # the derivation's premise
        if form == "wts":
            assert bool((~div[np.isin(rows.kind, (gn.ZERO_SUM, gn.NEG_SUM))]).all())
        for lanes in (16, 64):
            got = gn.pool_ref(c, form, renorm, lanes)
            assert got.shape == (c.B, c.H) and not got[~d.keeps].view(np.uint32).any()
            bad = gn.pool_mismatches_bound(got, ref, S, T, lanes)
            assert not bad, (c.name, form, renorm, lanes, gn.pool_bound(T, lanes), bad)
        if T <= 16:                                                        # one page either way: the same tree, the same bits
            assert not gc.mismatches_exact(gn.pool_ref(c, form, renorm, 16), gn.pool_ref(c, form, renorm, 64))


def test_pool_bound_is_the_derived_figure_and_sees_what_it_must():
    assert gn.tree_depth(16, 16) == 4 and gn.tree_depth(17, 16) == 5 and gn.tree_depth(64, 16) == 7
    assert gn.tree_depth(64, 64) == 6 and gn.tree_depth(65, 64) == 7 and gn.tree_depth(100, 64) == 7
    assert gn.pool_bound(16, 16) == 24 * 2.0 ** -24 and gn.pool_bound(100, 64) == 111 * 2.0 ** -24 < 7e-6
    c = next(c for c in gn.POOL_CASES if c.T == 16 and c.kernel == "four")
    d = gn.pool_data(c)
    ref, S, _, _ = _pool64(c, "counts", 1)
    good = gn.pool_ref(c, "counts", 1, 16)
    i = int(np.flatnonzero(d.keeps)[0])
    off = good.copy()
    off[i, 3] = np.nextafter(off[i, 3], np.float32(np.inf))                # one ulp: inside
    assert not gn.pool_mismatches_bound(off, ref, S, 16, 16)
    off[i, 3] = good[i, 3] + np.float32(1e-4) * np.float32(S[i, 3])        # a wrong weight: outside
    assert [m[:2] for m in gn.pool_mismatches_bound(off, ref, S, 16, 16)] == [(i, 3)]
    nan = good.copy()
    nan[0, 0] = np.nan
    assert [m[:2] for m in gn.pool_mismatches_bound(nan, ref, S, 16, 16)] == [(0, 0)]


def test_pool_ex_by_hand():
    """two rows worked by hand: the clamp of nvalid, tot over dropped entries, the fmaf chain, the renormalisation"""
    from oracle import c_oracle as co
    x = np.array([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], dtype=np.float32)
    ids = np.array([[0, 7, 1], [2, 1, -1]], dtype=np.int32)
    counts = np.array([[1, 2, 1], [3, 1, 9]], dtype=np.int32)
    nvalid = np.array([9, 2], dtype=np.int32)                              # 9 means 3
    f = np.float32
    out = co.pool_ex(x, ids, counts=counts, nvalid=nvalid, max_idx=1, renorm=False)
    assert out[0].tolist() == [f(0.25) * 1 + f(0.25) * 10, f(0.25) * 2 + f(0.25) * 20]          # tot = 4: id 7 counts in it
    assert out[1].tolist() == [2.5, 5.0]                                   # id 2 > max_idx dropped; 1 / (3 + 1) of row 1
    out = co.pool_ex(x, ids, counts=counts, nvalid=nvalid, max_idx=1, renorm=True)
    assert out[0].tolist() == [5.5, 11.0] and out[1].tolist() == [10.0, 20.0]
    w = np.array([[0.5, 3.0, -0.5], [1.0, 1.0, 1.0]], dtype=np.float32)
    out = co.pool_ex(x, ids, wts=w, nvalid=np.array([3, -1], dtype=np.int32), max_idx=99, renorm=True)      # max_idx above N - 1
    assert out[0].tolist() == [0.5 * 1 - 0.5 * 10, 0.5 * 2 - 0.5 * 20]     # sum 0: not renormalised; id 7 >= N dropped
    assert not out[1].view(np.uint32).any()                                # negative nvalid: +0
    with pytest.raises(RuntimeError):
        co.pool_ex(x, ids, nvalid=nvalid)                                  # neither counts nor weights


@pytest.mark.parametrize("c", gn.POOL_CASES, ids=lambda c: c.name)
def test_the_two_pool_oracles_agree_where_both_apply(c):
    """counts, renorm, max_idx = N - 1, 0 <= nvalid <= T, no negative id: orc_importance_pool (sequential weight sum, mul + add)
    and pool_ex differ by rounding only.  The case's rows with nvalid clipped to 0 .. T and every -1 pad written as the id N, which
    both drop (the older oracle knows no pads)."""
    from oracle import c_oracle as co
    d = gn.pool_data(c)
    rows, T = d.rows, c.T
    ids, counts, nvalid = np.where(rows.ids < 0, c.N, rows.ids).astype(np.int32), rows.counts, np.clip(rows.nvalid, 0, T)
    assert bool((nvalid > 0).sum() >= 16)
    old = co.importance_pool(d.x, ids, counts, nvalid, threads=2)
    ref, S, _, _ = gn.ref_pool64(d.x, ids, counts, None, nvalid, c.N - 1, True)
    for lanes in (16, 64):
        new = co.pool_ex(d.x, ids, counts=counts, nvalid=nvalid, max_idx=c.N - 1, renorm=True, lanes=lanes, threads=2)
        assert bool(new.any())
        bad = gn.pool_mismatches_bound(new, old.astype(np.float64), S, T, lanes)
        assert not bad, (c.name, lanes, bad)
