"""The dense GEMM's case table (tests/helpers/gemm_cases.py) proves itself here, without a GPU: every layout has the alignment
it claims, the runs of tests/test_hip_gemm_matrix.py reach every kernel instantiation launch_gemm can pick (by the restated
launcher -- a condition on shapes, flags and switches), the planted rows are what they are meant to be, and the derived norm
bound holds for a correct implementation: the C oracle's own fp32 normalisation stays inside it on every normalised case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_cases as gc  # noqa: E402


def test_case_names_are_unique_and_the_table_is_the_issue_s():
    names = [c.name for c in gc.CASES]
    assert len(set(names)) == len(names) == 16 + 18 + 4 + 5 + 2
    assert len(set(c.name for c in gc.LSH_CASES)) == len(gc.LSH_CASES) == 9
    assert gc.DMA_CASE in {c.name for c in gc.FAST_CASES}
    for c in gc.CASES:
        assert c.layout in gc.LAYOUTS and c.flagsets and c.M >= 1 and c.N >= 1 and c.K >= 2


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_layout_gives_the_alignment_it_claims(c):
    import torch
    d = gc.case_data(c)
    for big, W, K in ((d.Wbig, d.W, c.K), (d.W2big, d.W2, c.K2)):
        if K == 0:
            assert big is None and W is None
            continue
        off, ld = gc.claimed_alignment(K, c.layout)
        t = torch.from_numpy(big.copy())                                   # a fresh allocation, as the device tensor will be
        assert t.data_ptr() % 16 == 0
        v = gc.view_of(t, K, c.layout)
        assert tuple(v.shape) == (c.N, K) and v.stride(1) == 1 and (c.N == 1 or v.stride(0) == ld)
        assert v.data_ptr() % 16 == off and v.data_ptr() - t.data_ptr() == off
        assert np.array_equal(v.numpy(), W)                                # the view holds the oracle's W
        nv = gc.view_of(big, K, c.layout)
        assert nv.strides == (4 * ld, 4) and nv.ctypes.data - big.ctypes.data == off and np.shares_memory(nv, big)
        # what the layout is for: which of the launcher's alignment conditions it breaks
        if c.layout == "w_off1":
            assert off == 4 and ld % 4 == 0 and ld == K + 4
        elif c.layout == "ld33":
            assert off == 0 and ld % 4 != 0 and ld == K + 1
        else:
            assert off == 0 and ld == K
    fast = gc.is_fast(c.K, c.K2, c.layout)
    off, ld = gc.claimed_alignment(c.K, c.layout)
    assert fast == (off == 0 and ld % 4 == 0 and c.K % 32 == 0 and c.K2 % 32 == 0)
    assert ("FAST" in c.kernel or "pkernel" in c.kernel or "shard" in c.kernel) == fast and ("general" in c.kernel) == (not fast)


def test_every_way_to_lose_the_fast_path_is_in_the_table():
    """K % 32 == 0 and still not FAST: a weight view 4 bytes off (w_off1), ld % 4 != 0 (ld33); K % 32 != 0 with K % 4 == 0
    (load8 takes the float4 form) and with K % 4 != 0 (the scalar form); the same for K2"""
    slow = [c for c in gc.CASES if not gc.is_fast(c.K, c.K2, c.layout)]
    assert any(c.layout == "w_off1" and c.K % 32 == 0 and c.K2 % 32 == 0 for c in slow)
    assert any(c.layout == "ld33" and c.K % 32 == 0 and c.K2 % 32 == 0 for c in slow)
    assert any(c.layout == "plain" and c.K % 32 != 0 and c.K % 4 == 0 for c in slow)
    assert any(c.layout == "plain" and c.K % 4 != 0 for c in slow)
    assert any(c.K2 and c.K2 % 4 == 0 and c.K2 % 32 != 0 for c in slow) and any(c.K2 % 4 != 0 for c in slow)
    assert any(c.layout != "plain" and c.K2 for c in slow)


def test_recorded_kernel_is_the_launcher_s_default_choice():
    for c in gc.CASES:
        choices = {gc.launcher_choice(c.M, c.K, c.N, c.K2, c.layout, l2) for (_, l2) in c.flagsets}
        assert choices == {c.kernel}, (c.name, choices)


def test_the_runs_reach_every_instantiation():
    reached = set()
    for c in gc.CASES:
        for (_, l2) in c.flagsets:
            reached |= gc.kernels_of(gc.launcher_choice(c.M, c.K, c.N, c.K2, c.layout, l2))
    default = set(reached)
    for c in gc.FAST_CASES:
        for env, staged in gc.switch_runs(c):
            for (_, l2) in c.flagsets:
                reached |= gc.kernels_of(gc.launcher_choice(c.M, c.K, c.N, c.K2, c.layout, l2, env=env, staged=staged))
    assert reached == {
        "gemm_f32_kernel<2,2,1,1,FAST>", "gemm_f32_kernel<2,2,1,1,general>",
        "gemm_f32_kernel<2,2,1,2,FAST> one column tile", "gemm_f32_kernel<2,2,1,2,general> one column tile",
        "gemm_f32_kernel<2,2,1,2,FAST> several column tiles", "gemm_f32_kernel<2,2,1,2,general> several column tiles",
        "gemm_f32_kernel<1,4,1,2,FAST>", "gemm_f32_kernel<1,4,1,2,general>",
        "gemm_f32_kernel<1,4,2,2,FAST>", "gemm_f32_kernel<1,4,2,2,general>",
        "gemm_f32_pkernel<2,2,1,2>", "gemm_f32_pkernel<1,4,1,2>",
        "gemm_shard_kernel<ring 2, plain>", "gemm_shard_kernel<ring 2, WPERM>",
        "gemm_shard_kernel<ring 3, plain>", "gemm_shard_kernel<ring 3, WPERM>",
        "gemm_dma_kernel", "l2norm_rows_kernel"}
    assert reached == gc.INSTANTIATIONS
    # only a switch reaches these today (the persistent kernels and the ring take their shapes by default)
    assert gc.INSTANTIATIONS - default == {"gemm_f32_kernel<2,2,1,2,FAST> several column tiles", "gemm_f32_kernel<1,4,1,2,FAST>",
                                           "gemm_shard_kernel<ring 2, WPERM>", "gemm_shard_kernel<ring 3, WPERM>", "gemm_dma_kernel"}
    # the tile edges and size thresholds the table is there for
    by = {(c.M, c.N) for c in gc.CASES}
    assert {n for _, n in by} >= {1, 64, 65, 128, 129, 200, 256, 257}
    assert any(m > 16384 and n > 256 for m, n in by)                       # l2norm_rows_kernel: more rows than its 16 384 waves
    assert any(16384 < c.M < gc.MANY_ROWS and c.kernel == "gemm_f32_pkernel<1,4,1,2>" for c in gc.CASES)
    assert any(-(-c.M // 32) == 257 and "ring 2" in c.kernel for c in gc.CASES)
    # the LSH encode's runs: both tile widths, the persistent kernel, both rings, the general kernels
    lsh = set()
    for c in gc.LSH_CASES:
        d = gc.lsh_data(c)
        layout = "plain" if c.layout == "ld33" else c.layout               # ld33 goes in as a whole [nbits, D + 1] matrix
        lsh.add(gc.launcher_choice(c.n, d.D_call, c.nbits, 0, layout, False, lsh=True))
        if c in gc.LSH_FAST_CASES:
            for env in gc.LSH_SWITCHES:
                for staged in (False, True):
                    lsh.add(gc.launcher_choice(c.n, d.D_call, c.nbits, 0, layout, False, env=env, staged=staged, lsh=True))
    assert lsh >= {"gemm_f32_kernel<2,2,1,1,FAST>", "gemm_f32_kernel<2,2,1,1,general>", "gemm_f32_kernel<2,2,1,2,FAST> one column tile",
                   "gemm_f32_kernel<2,2,1,2,general> one column tile", "gemm_f32_kernel<2,2,1,2,general> several column tiles",
                   "gemm_f32_pkernel<2,2,1,2>", "gemm_shard_kernel<ring 2, plain>", "gemm_shard_kernel<ring 3, WPERM>"}


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_planted_rows_and_the_norm_bound_on_the_oracle(c):
    """The planted rows do what the table says, and -- for every case run with relu + l2 -- the oracle's own fp32 normalisation
    (sequential sum of squares, sqrtf, division) lies inside norm_bound(N) of the fp64 norm of its pre-norm output: the bound is
    not too tight for a correct implementation."""
    from oracle import c_oracle as co
    d = gc.case_data(c)
    raw = gc.ref_prenorm(c, False)
    assert raw.dtype == np.float32 and raw.shape == (c.M, c.N) and bool(np.isfinite(raw).all())
    if c.M >= 2:
        assert not d.x[0].any() and np.array_equal(raw[0], d.b)            # the zero row: the bias alone
    if c.M >= 3:
        assert bool((raw[1] < 0).all())                                    # every pre-activation negative
        relu = gc.ref_prenorm(c, True)
        assert not relu[1].view(np.uint32).any()                           # ... so ReLU leaves +0 bits
        assert c.N == 1 or bool(relu[2:].any(axis=1).all())                # and no other row is all zero (N = 1: about half are)
    assert bool(d.x[-1].all()) and bool(d.W[-1].all()) and bool((raw[-1] != d.b).all())      # the ragged edge is ordinary data
    for (relu, l2) in c.flagsets:
        if not l2:
            continue
        pre = gc.ref_prenorm(c, relu)
        got = co.linear(d.x, d.W, d.b, x2=d.x2, W2=d.W2, relu=relu, l2norm=True, threads=8)
        bad = gc.mismatches_normed(got, pre, gc.ref_normed_of(c, relu))
        assert not bad, (c.name, relu, gc.norm_bound(c.N), bad)
        if relu and c.M >= 3:
            assert not got[1].view(np.uint32).any()


def test_norm_bound_is_the_derived_figure():
    assert gc.norm_bound(256) == 131 * 2.0 ** -24 and 7.8e-6 < gc.norm_bound(256) < 7.9e-6 < 1e-5
    assert gc.norm_bound(129) == 67.5 * 2.0 ** -24
    # the checker sees what it must: one ulp at 1.0 is inside the bound at N = 129, a wrong norm is not; -0 in a zero row is not
    v = np.zeros((3, 129), dtype=np.float32)
    v[0, :4] = 0.5
    ref = gc.ref_normed(v)
    good = ref.astype(np.float32)
    assert not gc.mismatches_normed(good, v, ref)
    off = good.copy()
    off[0, 0] = np.nextafter(off[0, 0], np.float32(2.0))
    assert not gc.mismatches_normed(off, v, ref)
    off[0, 0] = good[0, 0] * np.float32(1.0 + 1e-5)
    assert gc.mismatches_normed(off, v, ref) == [(0, 0, float(off[0, 0]), 0.5)]
    neg = good.copy()
    neg[2, 7] = -0.0
    assert [m[:2] for m in gc.mismatches_normed(neg, v, ref)] == [(2, 7)]
    nan = good.copy()
    nan[1, 1] = np.nan
    assert [m[:2] for m in gc.mismatches_normed(nan, v, ref)] == [(1, 1)]
    a = np.array([[0.0, 1.0]], dtype=np.float32)
    assert [m[:2] for m in gc.mismatches_exact(np.array([[-0.0, 1.0]], dtype=np.float32), a)] == [(0, 0)]


@pytest.mark.parametrize("c", gc.LSH_CASES, ids=lambda c: c.name)
def test_lsh_cases_plant_exact_zero_dots(c):
    d = gc.lsh_data(c)
    codes = gc.lsh_ref(c)
    assert codes.shape == (c.n, c.nbits // 8) and c.nbits % 32 == 0
    assert bool((codes[0] == 0xff).all())                                  # the zero row: +0 >= 0 in every bit
    assert codes[1, 0] & 3 == 3                                            # (1, -1) . (1, 1) = +0 and (1, -1) . (-1, -1) = +0
    assert float(np.dot(d.x[1].astype(np.float64), d.A[0].astype(np.float64))) == 0.0
    bits = np.unpackbits(codes[2:], axis=1)
    assert 0.4 < bits.mean() < 0.6                                         # ordinary rows: both signs
    # what the call gets: a legal whole matrix whose rows are D_call apart, holding A
    A_call = d.A_store[d.A_first:d.A_first + c.nbits * d.D_call].reshape(c.nbits, d.D_call)
    assert np.array_equal(A_call[:, :c.D], d.A) and d.A_first + c.nbits * d.D_call <= d.A_store.size
    assert d.x_call.shape == (c.n, d.D_call) and np.array_equal(d.x_call[:, :c.D], d.x) and not d.x_call[:, c.D:].any()
    assert (d.A_first, d.D_call - c.D) == {"plain": (0, 0), "w_off1": (1, 0), "ld33": (0, 1)}[c.layout]
    if c.layout == "ld33":                                                 # the extra zero column changes no code
        from oracle import c_oracle as co
        assert np.array_equal(co.lsh_encode(d.x_call, A_call, threads=8), codes)
