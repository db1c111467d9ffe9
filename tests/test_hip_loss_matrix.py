"""The ranking losses (ps_hardest_negative, ps_margin_loss, ps_margin_loss_bwd: csrc/loss.hip and the row-arg-max epilogue of
csrc/dense_mfma.hip) against the C oracle, bit for bit -- never another GPU run.  tests/helpers/loss_cases.py holds the table
(ballot boundaries, column strides and passes, every grid cap, unaligned bases, the minimum shapes, a row without a candidate) and
tests/test_loss_cases.py proves on the CPU that each case produces its situation and that the comparison used here reports the
deviations a kernel could have.  The C ABI is called directly; every output is a view into a larger buffer of 0xFF bytes (a NaN
pattern for the floats) with at least 256 bytes of it on either side: after a call every output word equals the oracle's as an
integer, the bands are untouched, and a word that still holds the pattern is reported as not written."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import loss_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256                               # bytes of the fill pattern on either side of an output
TORCH_OF = {np.float32: torch.float32, np.int64: torch.int64, np.uint8: torch.uint8}


class Guarded:
    """an output of `shape` inside a buffer of 0xFF bytes"""

    def __init__(self, name, shape, dtype):
        self.name, self.dtype = name, dtype
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.buf = torch.full((GUARD + nbytes + GUARD,), lc.FILL, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD:GUARD + nbytes].view(TORCH_OF[dtype]).view(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + GUARD and self.t.data_ptr() % 16 == 0

    def numpy(self):
        return self.t.cpu().numpy()

    def bands(self):
        """lines for guard bytes that changed (empty: untouched)"""
        lo, hi = self.buf[:GUARD].cpu().numpy(), self.buf[-GUARD:].cpu().numpy()
        return [f"{self.name}: guard band {side} the output written at byte {int(np.flatnonzero(b != lc.FILL)[0])}"
                for side, b in (("before", lo), ("behind", hi)) if (b != lc.FILL).any()]


def _ptr(g):
    from pinsage_hip import native as nv
    return nv.ptr(None if g is None else g.t if isinstance(g, Guarded) else g)


def _place(a, unaligned):
    """a float32 array on the device: from the allocator (16-byte aligned), or a contiguous view one float behind such a base"""
    if a is None:
        return None
    t = torch.tensor(a)                                                       # a copy: the cached arrays are read-only
    if not unaligned:
        out = t.cuda()
        assert out.data_ptr() % 16 == 0
        return out
    base = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    out = base[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4 and base.data_ptr() % 16 == 0
    return out


def _operands(c, unaligned=None):
    d = lc.loss_data(c)
    un = c.unaligned if unaligned is None else unaligned
    return _place(d.Q, un), _place(d.P, un), _place(d.X, un)


def _forward(c, Q, P, X, what):
    """ps_hardest_negative + ps_margin_loss into guarded outputs -> (outputs by name, failure lines against the oracle)"""
    from pinsage_hip import native as nv
    fw = lc.c_forward(c)
    B, N, D = c.B, c.N, c.D
    out = {k: Guarded(k, (B,), t) for k, t in (("best", np.int64), ("sim", np.float32), ("idx (ps_hardest_negative)", np.int64),
                                               ("row_loss", np.float32), ("idx", np.int64), ("active", np.uint8))}
    out["loss"] = Guarded("loss", (1,), np.float32)
    flags = nv.PS_HN_PER_QUERY if c.mode == lc.PER_QUERY else nv.PS_HN_EXCLUDE_DIAG if c.mode == lc.BATCH_HARD else 0
    nv.call("ps_hardest_negative", _ptr(Q), B, D, _ptr(P if c.mode == lc.BATCH_HARD else X), N, flags, _ptr(out["best"]),
            _ptr(out["sim"]), _ptr(out["idx (ps_hardest_negative)"]), nv.stream())
    nv.call("ps_margin_loss", _ptr(Q), _ptr(P), B, D, _ptr(out["best"]), float(lc.loss_data(c).margin), _ptr(out["row_loss"]),
            _ptr(out["idx"]), _ptr(out["active"]), _ptr(out["loss"]), nv.stream())
    torch.cuda.synchronize()
    want = {"sim": fw.sim, "idx (ps_hardest_negative)": fw.idx, "row_loss": fw.row_loss, "idx": fw.idx, "active": fw.active,
            "loss": fw.loss}
    lines = []
    for k, g in out.items():
        lines += [f"{what}: {ln}" for ln in g.bands()]
        if k in want:
            lines += [f"{what}: {ln}" for ln in lc.report(c, k, g.numpy(), want[k])]
    return out, lines


def _backward(c, Q, P, X, go, names, x_arg=None):
    """ps_margin_loss_bwd over the ORACLE's idx / active for the outputs in `names` (the others NULL) -> guarded outputs"""
    from pinsage_hip import native as nv
    fw = lc.c_forward(c)
    shapes = {"dQ": (c.B, c.D), "dP": (c.B, c.D), "dX": (c.N, c.D) if c.mode == lc.SHARED else (c.B, c.N, c.D)}
    out = {k: Guarded(k, shapes[k], np.float32) for k in names}
    idx, active = torch.from_numpy(fw.idx.copy()).cuda(), torch.from_numpy(fw.active.copy()).cuda()
    g = torch.tensor([go], dtype=torch.float32).cuda()
    nv.call("ps_margin_loss_bwd", _ptr(Q), _ptr(P), _ptr(X if x_arg is None else x_arg), c.B, c.N, c.D, c.mode, _ptr(idx),
            _ptr(active), _ptr(g), _ptr(out.get("dQ")), _ptr(out.get("dP")), _ptr(out.get("dX")), nv.stream())
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), fw.idx) and np.array_equal(active.cpu().numpy(), fw.active)
    return out


def _grad_names(mode):
    return ("dQ", "dP") if mode == lc.BATCH_HARD else ("dQ", "dP", "dX")


def _backward_lines(c, out, go, what):
    fw, want = lc.c_forward(c), lc.c_backward(c, go)
    lines = []
    for k, g in out.items():
        scat = (fw.idx, fw.active) if k == lc.scatter_tensor(c.mode) else ()
        lines += [f"{what}, grad_out {go}: {ln}" for ln in g.bands() + lc.report(c, k, g.numpy(), want[k], *scat)]
    return lines


def _same_bits(a, b):
    return np.array_equal(lc._words(a), lc._words(b))


def _unchanged(c, Q, P, X):
    d = lc.loss_data(c)
    return all(t is None or _same_bits(t.cpu().numpy(), a) for t, a in ((Q, d.Q), (P, d.P), (X, d.X)))


@pytest.mark.parametrize("c", lc.CASES, ids=lambda c: c.name)
def test_losses_matrix_vs_oracle(c):
    from pinsage_hip import native as nv
    fw = lc.c_forward(c)
    Q, P, X = _operands(c)
    what = "unaligned bases" if c.unaligned else "aligned"
    outs, lines = _forward(c, Q, P, X, what)
    print(f"{c.name} forward: {'ok' if not lines else lines}")
    if c.unaligned:                                                           # the same data from the allocator: the same bits
        Qa, Pa, Xa = _operands(c, unaligned=False)
        outs_a, lines_a = _forward(c, Qa, Pa, Xa, "aligned")
        lines += lines_a
        lines += [f"case {c.name} ({c.reaches}): {k} differs between aligned and unaligned bases"
                  for k in outs if not _same_bits(outs[k].numpy(), outs_a[k].numpy())]
    if c.mode == lc.SHARED and c.B * c.N * c.D <= 1 << 25:                    # the per-query form on the expanded shared data
        X3 = X.unsqueeze(0).expand(c.B, -1, -1).contiguous()
        sim3, idx3 = Guarded("sim (per-query form)", (c.B,), np.float32), Guarded("idx (per-query form)", (c.B,), np.int64)
        best3 = Guarded("best", (c.B,), np.int64)
        nv.call("ps_hardest_negative", _ptr(Q), c.B, c.D, _ptr(X3), c.N, nv.PS_HN_PER_QUERY, _ptr(best3), _ptr(sim3), _ptr(idx3),
                nv.stream())
        torch.cuda.synchronize()
        lines += sim3.bands() + idx3.bands() + best3.bands()
        lines += lc.report(c, sim3.name, sim3.numpy(), fw.sim) + lc.report(c, idx3.name, idx3.numpy(), fw.idx)
        lines += [f"case {c.name} ({c.reaches}): {k} of the per-query form on the expanded data differs from the shared form"
                  for k, a, b in (("sim", sim3, "sim"), ("idx", idx3, "idx")) if not _same_bits(a.numpy(), outs[b].numpy())]
    if not _unchanged(c, Q, P, X):
        lines.append(f"case {c.name}: the forward changed an input")
    if lines:
        pytest.fail("\n".join(lines))
    if c.forward_only:
        return
    for go in c.gos:
        out = _backward(c, Q, P, X, go, _grad_names(c.mode))
        lines = _backward_lines(c, out, go, what)
        again = _backward(c, Q, P, X, go, _grad_names(c.mode))
        lines += [f"case {c.name} ({c.reaches}): {k} differs between two runs (grad_out {go})"
                  for k in out if not _same_bits(out[k].numpy(), again[k].numpy())]
        if c.unaligned:
            al = _backward(c, Qa, Pa, Xa, go, _grad_names(c.mode))
            lines += _backward_lines(c, al, go, "aligned")
            lines += [f"case {c.name} ({c.reaches}): {k} differs between aligned and unaligned bases (grad_out {go})"
                      for k in out if not _same_bits(out[k].numpy(), al[k].numpy())]
        print(f"{c.name} backward grad_out {go}: {'ok' if not lines else lines}")
        if not _unchanged(c, Q, P, X):
            lines.append(f"case {c.name}: the backward changed an input")
        if lines:
            pytest.fail("\n".join(lines))


def _subsets(names):
    return [s for n in range(1, len(names) + 1) for s in itertools.combinations(names, n)]


@pytest.mark.parametrize("mode", sorted(lc.NULL_SUBSET_CASES), ids=lambda m: lc.MODE_NAMES[m])
def test_null_subsets_of_the_gradients(mode):
    """every non-empty subset of the outputs the mode allows: what is requested equals the all-outputs run bit for bit, the guard
    bands and the inputs stay as they were.  Where the ABI lets X be NULL (batch-hard; dP alone) a small buffer of the fill pattern
    stands in its place and must come back untouched."""
    c = lc.BY_NAME[lc.NULL_SUBSET_CASES[mode]]
    Q, P, X = _operands(c)
    names = _grad_names(mode)
    go = c.gos[1]
    full = _backward(c, Q, P, X, go, names)
    lines = _backward_lines(c, full, go, "all outputs")
    for sub in _subsets(names):
        x_free = mode == lc.BATCH_HARD or sub == ("dP",)
        stand_in = Guarded("X stand-in", (64,), np.float32) if x_free else None
        out = _backward(c, Q, P, X, go, sub, x_arg=stand_in.t if x_free else None)
        assert set(out) == set(sub)
        lines += _backward_lines(c, out, go, f"outputs {sub}")
        lines += [f"case {c.name}: {k} of the run for {sub} differs from the all-outputs run"
                  for k in sub if not _same_bits(out[k].numpy(), full[k].numpy())]
        if stand_in is not None and (stand_in.bands() or (stand_in.buf.cpu().numpy() != lc.FILL).any()):
            lines.append(f"case {c.name}: the run for {sub} wrote to X")
        if not _unchanged(c, Q, P, X):
            lines.append(f"case {c.name}: the run for {sub} changed an input")
    if lines:
        pytest.fail("\n".join(lines))


@pytest.mark.parametrize("mode", sorted(lc.NULL_SUBSET_CASES), ids=lambda m: lc.MODE_NAMES[m])
def test_drop_ins_with_frozen_inputs(mode):
    """pinsage_hip.loss with requires_grad on each non-empty subset of (Q, P, X): the loss and the gradients are the C-ABI run's
    bits (grad_out 1.0), a frozen input has no gradient"""
    from pinsage_hip import loss as hl
    c = lc.BY_NAME[lc.NULL_SUBSET_CASES[mode]]
    d, fw, want = lc.loss_data(c), lc.c_forward(c), lc.c_backward(c, 1.0)
    Q0, P0, X0 = _operands(c)
    full = _backward(c, Q0, P0, X0, 1.0, _grad_names(mode))
    lines = _backward_lines(c, full, 1.0, "C ABI")
    inputs = ("Q", "P") if mode == lc.BATCH_HARD else ("Q", "P", "X")
    for sub in _subsets(inputs):
        t = {k: _place(a, False).requires_grad_(k in sub) for k, a in zip(("Q", "P", "X"), (d.Q, d.P, d.X)) if a is not None}
        if mode == lc.SHARED:
            loss = hl.max_margin_shared(t["Q"], t["P"], t["X"], d.margin)
        elif mode == lc.PER_QUERY:
            loss = hl.max_margin_per_query(t["Q"], t["P"], t["X"], d.margin)
        else:
            loss = hl.batch_hard(t["Q"], t["P"], d.margin)
        lines += lc.report(c, f"loss (drop-in, requires_grad on {sub})", loss.detach().reshape(1).cpu().numpy(), fw.loss)
        loss.backward()
        for k in inputs:
            if k not in sub:
                if t[k].grad is not None:
                    lines.append(f"case {c.name}: frozen {k} received a gradient (requires_grad on {sub})")
                continue
            got = t[k].grad.cpu().numpy()
            lines += lc.report(c, f"d{k} (drop-in, requires_grad on {sub})", got, want[f"d{k}"])
            if not _same_bits(got, full[f"d{k}"].numpy()):
                lines.append(f"case {c.name}: d{k} of the drop-in (requires_grad on {sub}) differs from the C-ABI run")
    if lines:
        pytest.fail("\n".join(lines))
