"""Every tile form of the dense GEMM (csrc/dense_mfma.hip: ps_linear, ps_lsh_encode) against the C oracle's k-ordered fmaf chain
at ragged shapes.  tests/helpers/gemm_cases.py holds the table -- the smallest shapes that reach each instantiation launch_gemm
can pick, with a last row / column tile that is partly empty, unaligned and strided weight views, planted zero and all-negative
rows -- and tests/test_gemm_cases.py proves on the CPU that the runs made here reach all of them and that the norm bound holds
for the oracle itself.  Before the norm every output must equal the oracle's bits; after it, the fp64 norm of those bits within
the derived bound norm_bound(N), rows that are zero before the norm as +0.  The reference is the oracle in every run, never
another GPU run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCH_NAMES = ("PS_GEMM_SHARD", "PS_GEMM_PERSIST", "PS_GEMM_DMA")


def _device_operands(c):
    """x, W, b, x2, W2 on the device; W / W2 are the views of the case's layout, handed to the kernel without a copy"""
    from pinsage_hip import dense
    d = gc.case_data(c)
    dev = lambda a: None if a is None else torch.tensor(a).cuda()          # noqa: E731  (a copy: the cached arrays are read-only)
    x, b, x2 = dev(d.x), dev(d.b), dev(d.x2)
    views = []
    for big, K in ((d.Wbig, c.K), (d.W2big, c.K2)):
        if K == 0:
            views.append(None)
            continue
        t = dev(big)
        v = gc.view_of(t, K, c.layout)
        off, ld = gc.claimed_alignment(K, c.layout)
        assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == off and (c.N == 1 or v.stride(0) == ld) and v.stride(1) == 1
        kept, ldk = dense._rowmajor(v)
        assert kept.data_ptr() == v.data_ptr() and ldk == ld               # dense.linear passes the view itself
        views.append(v)
    return x, views[0], b, x2, views[1]


def _check_linear(c, ops, env=(), staged=False):
    """every flag set of case c under the switches in env (already set), against the oracle"""
    from pinsage_hip import dense
    x, W, b, x2, W2 = ops
    if staged:
        W, W2 = dense.stage_weight(W), dense.stage_weight(W2)
        assert isinstance(W, dense.StagedWeight) and (W2 is None or isinstance(W2, dense.StagedWeight))
    for (relu, l2) in c.flagsets:
        y = dense.linear(x, W, b, x2=x2, W2=W2, relu=relu, l2norm=l2)
        got = y.cpu().numpy()
        assert got.shape == (c.M, c.N)
        pre = gc.ref_prenorm(c, relu)
        bad = gc.mismatches_normed(got, pre, gc.ref_normed_of(c, relu)) if l2 else gc.mismatches_exact(got, pre)
        kernel = gc.launcher_choice(c.M, c.K, c.N, c.K2, c.layout, l2, env=env, staged=staged)
        print(f"{c.name} relu={relu} l2={l2} env={dict(env)} staged={staged}: {kernel}: {'ok' if not bad else bad}")
        assert not bad, (f"case {c.name}, relu={relu}, l2={l2}, switches {dict(env)}, image-order weights {staged}; expected kernel "
                         f"{kernel}; first (row, col, got, want): {bad}" + (f"; bound {gc.norm_bound(c.N):.3e} relative" if l2 else ""))


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_linear_matrix_vs_oracle(c, monkeypatch):
    for name in SWITCH_NAMES:
        monkeypatch.delenv(name, raising=False)
    _check_linear(c, _device_operands(c))


@pytest.mark.parametrize("c", gc.FAST_CASES, ids=lambda c: c.name)
def test_linear_matrix_under_every_launcher_switch(c, monkeypatch):
    """The launcher's default choice can change; a switch pins an instantiation.  The aligned cases again under PS_GEMM_SHARD =
    0 / 2 / 3, PS_GEMM_PERSIST=0 (with PS_GEMM_SHARD=0: the one-tile kernels), PS_GEMM_DMA=1 (the one case it serves), each with
    plain and image-order weights (dense.stage_weight).  launch_gemm reads the environment on every launch."""
    ops = _device_operands(c)
    for env, staged in gc.switch_runs(c):
        for name in SWITCH_NAMES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env:
            monkeypatch.setenv(name, value)
        _check_linear(c, ops, env=env, staged=staged)


def _check_lsh(c, got, what):
    want = gc.lsh_ref(c)
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    assert bool((got[0] == 0xff).all()), f"{c.name} {what}: the all-zero row must encode as all ones (+0 >= 0)"
    assert got[1, 0] & 3 == 3, f"{c.name} {what}: dots of exactly +0 must encode as 1"
    gb, wb = np.unpackbits(got, axis=1, bitorder="little"), np.unpackbits(want, axis=1, bitorder="little")
    bad = np.argwhere(gb != wb)
    assert bad.size == 0, (f"case {c.name} {what}: {bad.shape[0]} bits differ; first (row, bit, got, want): "
                           f"{[(int(r), int(j), int(gb[r, j]), int(wb[r, j])) for r, j in bad[:8]]}")


@pytest.mark.parametrize("c", gc.LSH_CASES, ids=lambda c: c.name)
def test_lsh_encode_matrix_vs_oracle(c, monkeypatch):
    """dense.lsh_encode / ps_lsh_encode (the GEMM with the sign + ballot epilogue) against the oracle, bit-exact: every tile width,
    D % 32 != 0 and D % 4 != 0, an unaligned A, planted dots of exactly +0.  dense.lsh_encode copies a strided A, and the C entry
    point has no leading dimension for it, so the w_off1 / ld33 cases call ps_lsh_encode through native.call with flags 0, the
    view's own pointer and a D that makes the view a legal whole matrix (helpers/gemm_cases.lsh_data says which)."""
    from pinsage_hip import dense, native as nv
    for name in SWITCH_NAMES:
        monkeypatch.delenv(name, raising=False)
    d = gc.lsh_data(c)
    x = torch.tensor(d.x_call).cuda()
    store = torch.tensor(d.A_store).cuda()
    A = store[d.A_first:d.A_first + c.nbits * d.D_call].view(c.nbits, d.D_call)
    assert store.data_ptr() % 16 == 0 and A.data_ptr() % 16 == 4 * d.A_first and A.is_contiguous()
    layout = "plain" if c.layout == "ld33" else c.layout
    if c.layout == "plain":
        _check_lsh(c, dense.lsh_encode(x, A), "default")
    else:
        codes = torch.empty((c.n, c.nbits // 8), dtype=torch.uint8, device="cuda")
        nv.call("ps_lsh_encode", nv.ptr(x), nv.i64(c.n), nv.i32(d.D_call), nv.ptr(A), nv.i32(c.nbits), nv.ptr(codes), nv.i32(0),
                nv.stream())
        _check_lsh(c, codes, gc.launcher_choice(c.n, d.D_call, c.nbits, 0, layout, False, lsh=True))
    if c in gc.LSH_FAST_CASES:
        S = dense.stage_weight(A)
        assert isinstance(S, dense.StagedWeight)
        _check_lsh(c, dense.lsh_encode(x, S), "image-order A")
        for env in gc.LSH_SWITCHES:
            for name, value in env:
                monkeypatch.setenv(name, value)
            for staged in (False, True):
                what = gc.launcher_choice(c.n, d.D_call, c.nbits, 0, layout, False, env=env, staged=staged, lsh=True)
                _check_lsh(c, dense.lsh_encode(x, S if staged else A), f"{dict(env)} {what}")
