"""Ranking losses over libpinsage_hip.so: loss = mean_b relu((margin + max_j q_b . x_j) - q_b . p_b) and its gradient from ONE
(maximum, arg-max) pair per query row.

forward : ps_hardest_negative (shared candidates: ps_linear's fp32-MFMA tiles with a row-arg-max epilogue; per-query candidates:
          a streaming kernel) + ps_margin_loss (positive similarity, hinge, active mask, fixed-shape mean): two library calls.
backward: ps_margin_loss_bwd, the closed form over the arg-max indices (include/pinsage_hip.h): one library call.

The autograd state is (Q, P, X, idx, active): O(B) beyond the inputs, never a [B, N] or [B, N, D] tensor.  The backward is
once_differentiable: a double backward raises.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import native as nv

SHARED, PER_QUERY, BATCH_HARD = nv.PS_LOSS_SHARED, nv.PS_LOSS_PER_QUERY, nv.PS_LOSS_BATCH_HARD


def _fp32_cuda(name, t, dim):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise nv.NativeError(f"{name}: device (HBM) tensor expected (no CPU fallback in pinsage_hip.loss)")
    if t.dtype != torch.float32 or t.dim() != dim:
        raise TypeError(f"{name}: fp32 tensor with {dim} dimensions expected, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _check_shapes(Q, X, mode):
    B, D = int(Q.size(0)), int(Q.size(1))
    if mode == PER_QUERY:
        if int(X.size(0)) != B or int(X.size(2)) != D:
            raise ValueError(f"shape mismatch: Q {tuple(Q.shape)} vs per-query candidates {tuple(X.shape)}")
        N = int(X.size(1))
    else:
        if int(X.size(1)) != D:
            raise ValueError(f"shape mismatch: Q {tuple(Q.shape)} vs candidates {tuple(X.shape)}")
        N = int(X.size(0))
    if B == 0 or N == 0:
        raise ValueError("at least one query row and one candidate expected")
    return B, N, D


def _best(Q, X, mode, exclude_diag, sim=None, idx=None):
    """the packed (maximum, arg-max) words of ps_hardest_negative, uint64 [B] held in an int64 tensor"""
    B, N, D = _check_shapes(Q, X, mode)
    best = torch.empty(B, dtype=torch.int64, device=Q.device)
    flags = (nv.PS_HN_PER_QUERY if mode == PER_QUERY else 0) | (nv.PS_HN_EXCLUDE_DIAG if exclude_diag else 0)
    with torch.cuda.device(Q.device):
        nv.call("ps_hardest_negative", nv.ptr(Q), B, D, nv.ptr(X), N, flags, nv.ptr(best), nv.ptr(sim), nv.ptr(idx), nv.stream())
    return best


def hardest_negative(Q, X, exclude_diag=False):
    """-> (sim fp32 [B], idx int64 [B]): per row of Q [B, D] the largest similarity to a candidate and the smallest index that
    attains it.  X [N, D]: candidates shared by all rows -- sim[b] is bit-identical to dense.linear(Q, X)[b, idx[b]], the
    [B, N] matrix is never written; exclude_diag leaves candidate j == b out (-inf / -1 for a row without a candidate).
    X [B, N, D]: row b sees X[b] only; bit-identical to the shared form on equal data.  A NaN similarity is its row's maximum."""
    Q = _fp32_cuda("Q", Q, 2)
    mode = PER_QUERY if isinstance(X, torch.Tensor) and X.dim() == 3 else SHARED
    X = _fp32_cuda("X", X, 3 if mode == PER_QUERY else 2)
    if exclude_diag and mode == PER_QUERY:
        raise ValueError("exclude_diag applies to shared candidates")
    sim = torch.empty(int(Q.size(0)), dtype=torch.float32, device=Q.device)
    idx = torch.empty(int(Q.size(0)), dtype=torch.int64, device=Q.device)
    _best(Q, X, mode, exclude_diag, sim, idx)
    return sim, idx


class _MarginLoss(torch.autograd.Function):
    """mode SHARED: X [N, D]; PER_QUERY: X [B, N, D]; BATCH_HARD: X is None (the candidates are the positives, j != b)"""

    @staticmethod
    def forward(ctx, Q, P, X, mode, margin):
        Q, P = _fp32_cuda("Q", Q, 2), _fp32_cuda("P", P, 2)
        if P.shape != Q.shape:
            raise ValueError(f"shape mismatch: Q {tuple(Q.shape)} vs P {tuple(P.shape)}")
        if mode == BATCH_HARD:
            X = None
        else:
            X = _fp32_cuda("X", X, 3 if mode == PER_QUERY else 2)
        best = _best(Q, P if X is None else X, mode, mode == BATCH_HARD)
        B, D = int(Q.size(0)), int(Q.size(1))
        dev = Q.device
        row_loss = torch.empty(B, dtype=torch.float32, device=dev)
        idx = torch.empty(B, dtype=torch.int64, device=dev)
        active = torch.empty(B, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nv.call("ps_margin_loss", nv.ptr(Q), nv.ptr(P), B, D, nv.ptr(best), float(margin), nv.ptr(row_loss), nv.ptr(idx),
                    nv.ptr(active), nv.ptr(loss), nv.stream())
        ctx.mode = mode
        ctx.save_for_backward(Q, P, X, idx, active)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        Q, P, X, idx, active = ctx.saved_tensors
        mode = ctx.mode
        B, D = int(Q.size(0)), int(Q.size(1))
        N = B if X is None else int(X.size(1 if mode == PER_QUERY else 0))
        need_q, need_p, need_x = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and X is not None
        dQ = torch.empty_like(Q) if need_q else None
        dP = torch.empty_like(P) if need_p else None
        dX = torch.empty_like(X) if need_x else None
        go = grad_out.to(device=Q.device, dtype=torch.float32).reshape(1).contiguous()
        with torch.cuda.device(Q.device):
            nv.call("ps_margin_loss_bwd", nv.ptr(Q), nv.ptr(P), nv.ptr(X), B, N, D, mode, nv.ptr(idx), nv.ptr(active), nv.ptr(go),
                    nv.ptr(dQ), nv.ptr(dP), nv.ptr(dX), nv.stream())
        return dQ, dP, dX, None, None


def max_margin_shared(Q, P, X, margin=0.1):
    """mean_b relu((margin + max_j Q_b . X_j) - Q_b . P_b) with candidates X [N, D] shared by the batch; 0-dim fp32, on the tape"""
    return _MarginLoss.apply(Q, P, X, SHARED, margin)


def max_margin_per_query(Q, P, X, margin=0.1):
    """the same with row b's own candidates X[b] of X [B, N, D]"""
    return _MarginLoss.apply(Q, P, X, PER_QUERY, margin)


def batch_hard(Q, P, margin=0.1):
    """the same with the other rows' positives as candidates: max over j != b of Q_b . P_j"""
    return _MarginLoss.apply(Q, P, None, BATCH_HARD, margin)


def forward_state(Q, P, X, mode, margin=0.1):
    """(loss, idx int64 [B], active bool [B]) of one forward, off the tape: what the backward is a closed form of (tests, probes)"""
    with torch.no_grad():
        class _Ctx:
            def save_for_backward(self, *t):
                self.saved = t
        ctx = _Ctx()
        loss = _MarginLoss.forward(ctx, Q, P, X, mode, margin)
    return loss, ctx.saved[3], ctx.saved[4].bool()
