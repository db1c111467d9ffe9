"""The special-value table (tests/helpers/special_cases.py) proves itself here, without a GPU: its cases reach every kernel
instantiation, every planting produces the class it is there for in the oracle's output, the planted rows share a 32-row MFMA
block with ordinary rows, torch's fp64 expression agrees with the oracle about every class up to the named deviations, and the
selects the GEMM's epilogue had before -- which dropped a NaN -- disagree with the table on named cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_cases as gc  # noqa: E402
import special_cases as sc  # noqa: E402

ORDINARY_ROWS = (2, 4, 7, 8, 11, 13)                       # of the first 32-row block, beside the planted ones
RUNS = [(c, v) for c in sc.BASES for v in sc.VARIANTS]
RUN_IDS = [f"{c.name}-{v}" for c, v in RUNS]


def _is(a, cls):
    return sc.classes(a) == cls


def test_the_cases_reach_every_instantiation_and_are_the_smallest_that_do():
    reached = set()
    for c in sc.BASES:
        assert sc.eligible(c)
        reached |= set(sc.reached_by(c))
    assert reached == gc.INSTANTIATIONS == set(sc.CHOSEN)
    for inst, c in sc.CHOSEN.items():
        assert inst in sc.reached_by(c)
        rivals = [o for o in gc.CASES if sc.eligible(o) and inst in sc.reached_by(o)]
        by_default = lambda o: sc.reached_by(o)[inst][:2] == ((), False)   # noqa: E731
        pool = [o for o in rivals if by_default(o)] or rivals              # the launcher's own choice before a switch
        assert c in pool and all(o.M * o.N * (o.K + o.K2) >= c.M * c.N * (c.K + c.K2) for o in pool), (inst, c.name)
    # the switch runs of the FAST bases reach what only a switch reaches
    only_switch = {i for i, c in sc.CHOSEN.items() if sc.reached_by(c)[i][:2] != ((), False)}
    assert only_switch == {"gemm_f32_kernel<2,2,1,2,FAST> several column tiles", "gemm_f32_kernel<1,4,1,2,FAST>",
                           "gemm_shard_kernel<ring 2, WPERM>", "gemm_shard_kernel<ring 3, WPERM>", "gemm_dma_kernel"}
    assert all(sc.CHOSEN[i] in sc.FAST_BASES for i in only_switch)
    assert sc.NORM_ROWS_BASE.N > 256 and gc.RELU_L2 in sc.NORM_ROWS_BASE.flagsets
    assert any(c.K2 for c in sc.BASES) and any(not c.K2 for c in sc.BASES)
    assert any(c.K % 32 for c in sc.BASES) and any(c.K2 % 32 for c in sc.BASES)          # a ragged last K step, of x and of x2


def test_the_chain_that_ends_in_minus_zero():
    """fmaf(-1e-30, 1e-30, +0.0) rounds to -0.0 (the exact product, -1e-60, is below half the smallest subnormal), and
    -0.0 + -0.0 is -0.0, where + 0.0f gives +0.0"""
    from oracle import c_oracle as co
    exact = float(-sc.TINY) * float(sc.TINY) + 0.0                         # exact in fp64
    assert exact < 0 and abs(exact) < 2.0 ** -150
    r = np.float32(exact)
    assert r == 0 and np.signbit(r)
    x, W = np.zeros((1, 32), dtype=np.float32), np.full((1, 32), 0.7, dtype=np.float32)
    x[0, 31], W[0, 31] = -sc.TINY, sc.TINY
    word = lambda b, relu, K=32: int(co.linear(x[:, 32 - K:], W[:, 32 - K:], b, relu=relu).view(np.uint32)[0, 0])     # noqa: E731
    neg0 = np.array([-0.0], dtype=np.float32)
    assert word(neg0, False) == 0x80000000                                 # -0.0 stored
    assert word(neg0, True) == 0                                           # PS_RELU: t > 0 or NaN ? t : +0.0
    assert word(None, False) == 0 and word(None, True) == 0                # a null bias is + 0.0f
    assert word(np.zeros(1, dtype=np.float32), False) == 0
    # a chain whose length is no multiple of 32 runs on over +0.0 * +0.0 (the kernel's K step is padded): -0.0 + +0.0 = +0.0
    assert word(neg0, False, K=31) == 0 and word(neg0, False, K=2) == 0


@pytest.mark.parametrize("c", sc.BASES, ids=lambda c: c.name)
def test_planted_rows_share_an_mfma_block_with_ordinary_rows(c):
    rows = sc.planted_rows(c)
    head = {r for n, r in rows.items() if n != "nan_tail"}
    assert len(set(rows.values())) == len(rows) and not head & {0, 1, c.M - 1} and not head & set(ORDINARY_ROWS)
    assert all(r // 32 == 0 for r in head | set(ORDINARY_ROWS)) and max(ORDINARY_ROWS) < c.M - 1
    if "nan_tail" in rows:                                                 # far from the others, the last row behind it ordinary
        assert rows["nan_tail"] == c.M - 2 > 31
    cols = (sc.C_OVP, sc.C_NEG0, sc.C_WNAN, sc.C_OVN, sc.C_BNAN)
    assert len(set(cols)) == 5 and max(cols) < c.N - 1 and max(cols) // 32 == 0
    d, base = sc.data(c, "rows"), gc.case_data(c)
    for r in ORDINARY_ROWS + (0, 1, c.M - 1):                              # untouched: the table's data
        assert np.array_equal(d.x[r], base.x[r]) and (c.K2 == 0 or np.array_equal(d.x2[r], base.x2[r]))
    for relu, l2 in c.flagsets:
        y = sc.expected(c, "rows", relu, l2)
        assert bool(np.isfinite(y[list(ORDINARY_ROWS)]).all()) and bool(np.isfinite(y[[0, 1, c.M - 1]]).all())
    # the NaN sits inside the last K step, the values of a case live in float operands only
    assert c.K - 1 >= (c.K - 1) // 32 * 32 and np.isnan(d.x[sc.R_NAN, c.K - 1]) and np.isnan(d.x[sc.R_NAN]).sum() == 1


@pytest.mark.parametrize("c", sc.BASES, ids=lambda c: c.name)
def test_every_planting_produces_its_class_in_the_oracle(c):
    rows, d = sc.planted_rows(c), sc.data(c, "rows")
    w = d.W[:, sc.K_INF]
    assert bool((w > 0).any()) and bool((w < 0).any()) and bool((w != 0).all())          # +Inf against both signs
    others = np.delete(np.abs(d.W[:, sc.K_OVF]), [sc.C_OVP, sc.C_OVN])
    assert others.max() < 1.13 and float(sc.BIG) * 1.13 < 3.4028e38 < float(sc.BIG) * 1.5
    w2 = d.W2[:, sc.K_INF] if c.K2 else d.W[:, sc.K_INF2]
    clash = np.sign(w) == np.sign(w2)                                      # Inf - Inf where the two weights have one sign
    assert bool(clash.any()) and bool((~clash).any()) and bool((w2 != 0).all())
    planted = sorted(rows.values())
    rest = np.setdiff1d(np.arange(c.M), planted)
    for variant in ("rows", "rows_nobias"):
        for relu, l2 in c.flagsets:
            y = sc.expected(c, variant, relu, l2)
            assert bool(np.isfinite(y[rest]).all()), "poison outside the planted rows"
            for name in ("nan", "nan2", "nan_tail"):
                if name in rows:
                    assert bool(np.isnan(y[rows[name]]).all()), (name, relu, l2)
            yi, yii, yo, yz = y[sc.R_INF], y[sc.R_INFINF], y[sc.R_OVF], y[sc.R_NEG0]
            if not l2:
                assert bool(_is(yi[w > 0], sc.PINF).all()) and bool(_is(yi[w < 0], sc.PZERO if relu else sc.NINF).all())
                assert bool(np.isnan(yii[clash]).all()) and bool(np.isinf(yii[~clash] if not relu else yii[~clash & (w > 0)]).all())
                assert _is(yo[sc.C_OVP], sc.PINF) and _is(yo[sc.C_OVN], sc.PZERO if relu else sc.NINF)
                assert bool(np.isfinite(np.delete(yo, [sc.C_OVP, sc.C_OVN])).all())
            else:
                assert bool(np.isnan(yi[w > 0]).all()) and bool((_is(yi[w < 0], sc.PZERO) if relu else np.isnan(yi[w < 0])).all())
                assert bool(np.isnan(yii).all())                           # a NaN norm: the clamp leaves it, x / NaN
                assert np.isnan(yo[sc.C_OVP]) and (_is(yo[sc.C_OVN], sc.PZERO) if relu else np.isnan(yo[sc.C_OVN]))
                fin = np.delete(yo, [sc.C_OVP, sc.C_OVN])
                assert bool((fin == 0).all())                              # finite / Inf = +-0
            want0 = sc.NZERO if (variant == "rows" and not relu and sc.neg0_survives(c)) else sc.PZERO
            assert _is(yz[sc.C_NEG0], want0), (variant, relu, l2, yz[sc.C_NEG0])
            assert bool(np.isfinite(yz).all()) and bool(yz.any())          # the row has a norm: the sign went through a division
    for variant, col in (("w_nan", sc.C_WNAN), ("b_nan", sc.C_BNAN)):
        for relu, l2 in sc.flagsets_of(c, variant):
            assert not l2
            y = sc.expected(c, variant, relu, l2)
            assert bool(np.isnan(y[:, col]).all()) and bool(np.isfinite(np.delete(y, col, axis=1)).all())
            assert not sc.data(c, variant).x[0].any()                      # the all-zero row is poisoned too: 0 * NaN


@pytest.mark.parametrize("c,variant", RUNS, ids=RUN_IDS)
def test_torch_fp64_agrees_with_the_oracle_about_every_class(c, variant):
    """F.normalize(F.relu(x @ W.T + x2 @ W2.T + b)) in fp64 on the CPU, rounded to fp32 (which turns -1e-60 into -0.0 as the fmaf
    does), has the oracle's class in every planted row and column.  Named deviations:
      NEG0      ps_linear turns -0.0 into +0.0 where torch keeps it: relu(-0.0) (checked below on the oracle's own pre-activation,
                which fp64 never rounds to -0.0 before the ReLU), the null bias's + 0.0f and the + 0.0 * 0.0 terms behind a chain
                whose length is no multiple of 32;
      OVERFLOW  fp64 does not overflow where fp32 does, so with the norm row R_OVF is held to the expression in fp32.
    Ordinary outputs are held by the ordinary cases; here they must only stay ordinary (a sum near zero may round to either
    side of it in the two precisions)."""
    import torch
    import torch.nn.functional as F
    rows = sorted(sc.planted_rows(c).values()) + [0, 1] if variant.startswith("rows") else []
    cols = [] if variant.startswith("rows") else [sc.C_WNAN if variant == "w_nan" else sc.C_BNAN]
    for relu, l2 in sc.flagsets_of(c, variant):
        ec = sc.classes(sc.expected(c, variant, relu, l2))
        tc = sc.torch_classes(c, variant, relu, l2)
        if variant.startswith("rows") and l2:
            tc[sc.R_OVF] = sc.torch_classes(c, variant, relu, l2, dtype="float32")[sc.R_OVF]            # OVERFLOW
        if variant.startswith("rows") and not relu and (variant == "rows_nobias" or not sc.neg0_survives(c)):   # NEG0: + 0.0
            assert tc[sc.R_NEG0, sc.C_NEG0] == sc.NZERO and ec[sc.R_NEG0, sc.C_NEG0] == sc.PZERO
            tc[sc.R_NEG0, sc.C_NEG0] = sc.PZERO
        held = np.zeros(ec.shape, dtype=bool)
        held[rows] = True
        held[:, cols] = True
        bad = np.argwhere(held & (tc != ec))
        assert bad.size == 0, (c.name, variant, relu, l2, [(int(r), int(q), sc.CLASS_NAMES[tc[r, q]], sc.CLASS_NAMES[ec[r, q]])
                                                            for r, q in bad[:8]])
        ordinary = (sc.FINITE, sc.PZERO, sc.NZERO)
        assert bool(np.isin(tc[~held], ordinary).all()) and bool(np.isin(ec[~held], ordinary).all())
        if relu and not l2:                                                                             # NEG0: relu(-0.0)
            pre = sc.expected(c, variant, False, False)
            t = F.relu(torch.tensor(pre)).numpy()
            differ = np.argwhere(sc.classes(t) != ec)
            want = [[sc.R_NEG0, sc.C_NEG0]] if variant == "rows" and sc.neg0_survives(c) else []
            assert differ.tolist() == want and all(pre.view(np.uint32)[r, q] == 0x80000000 for r, q in want)


@pytest.mark.parametrize("c", sc.BASES, ids=lambda c: c.name)
def test_the_selects_that_drop_a_nan_are_caught(c):
    """orc_linear with v > 0 ? v : 0 and nrm > 1e-12f ? nrm : 1e-12f (special_cases.slipped) disagrees with the table: under the
    ReLU every NaN of x, W and b comes out +0.0; under the norm alone the row whose columns are NaN and Inf side by side comes
    out +-Inf instead of NaN.  Without either flag nothing differs: the slip is in the two selects alone."""
    rows = sc.planted_rows(c)
    for variant in sc.VARIANTS:
        for relu, l2 in sc.flagsets_of(c, variant):
            got = sc.slipped(c, variant, relu, l2)
            bad = {(r, q) for r, q, _, _ in sc.mismatches(got, sc.expected(c, variant, relu, l2),
                                                          sc.expected_ref64(c, variant, relu) if l2 else None, limit=None)}
            if not relu and not l2:
                assert not bad, (c.name, variant, sorted(bad)[:4])
            elif variant == "w_nan":
                assert bad == {(r, sc.C_WNAN) for r in range(c.M)}
            elif variant == "b_nan":
                assert bad == {(r, sc.C_BNAN) for r in range(c.M)}
            else:
                bad_rows = {r for r, _ in bad}
                assert sc.R_INFINF in bad_rows, (c.name, variant, relu, l2)
                if relu:
                    assert bad_rows >= {rows[n] for n in ("nan", "nan2", "nan_tail") if n in rows}
                assert bad_rows <= set(rows.values())


@pytest.mark.parametrize("N", sc.EPI_N)
def test_epilogue_backward_restatement_agrees_with_torch_about_every_class(N):
    """linear_bwd_cases.epilogue_bwd_exact on the planted activations (a NaN row, an Inf row, rows at the clamp, a -0.0, a NaN in
    g) has the class of torch's fp64 autograd of F.normalize(F.relu(z)) in every element, up to MASK_NAN"""
    from helpers import linear_bwd_cases as lb
    t, g, rows = sc.epilogue_special(N)
    assert np.isinf(t[rows["inf_row"]]).sum() == 1 and np.isnan(g).sum() == 1 and np.isnan(t).sum() == 1
    assert np.signbit(t[rows["neg0_row"], min(1, N - 1)]) and t[rows["neg0_row"], min(1, N - 1)] == 0
    for relu, l2 in lb.FLAGSETS:
        gz = lb.epilogue_bwd_exact(t, g, relu, l2, lb.vec_of(N))
        assert sc.epilogue_class_mismatches(gz, t, g, relu, l2) == [], (N, relu, l2)
        poisoned = np.isnan(gz).any(axis=1)
        want = {rows["gnan_row"]} | ({rows["nan_row"], rows["inf_row"]} if l2 else set())       # without the norm gz is g, masked
        assert set(np.flatnonzero(poisoned)) == want, (N, relu, l2)
