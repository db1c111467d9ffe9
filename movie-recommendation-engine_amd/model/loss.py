"""model.loss -- drop-in for the reference module of the same name (reference model/loss.py): MaxMarginRankingLoss,
BatchHardTripletLoss and CurriculumLoss with the reference's constructors, attributes and forward signatures, computed on the
device from one (largest negative similarity, arg-max) pair per query row (pinsage_hip.loss).

    loss = mean_b relu(margin + max_j q_b . x_j - q_b . p_b)

Where the negatives come from decides the kernel:
  * [B, N, D] whose batch stride is 0 -- `neg.unsqueeze(0).expand(B, -1, -1)`, the sampler's shared negatives passed through the
    reference's signature: ONE fp32-MFMA product Q X^T with a row-arg-max epilogue on the [N, D] tensor the caller expanded.  The
    tape is routed to that tensor (the view's `_base`), so the gradient arrives as [N, D]; nothing of size [B, N] or [B, N, D]
    exists in either direction.  A view without a usable base takes the next path.
  * any other [B, N, D]: per-query candidates, a streaming kernel that reads every row once.
  * [B, D]: one negative per query (the same kernel with N = 1).
  * BatchHardTripletLoss: the other rows' positives, Q P^T with the diagonal left out.
fp32 CUDA tensors take the device path; anything else (CPU tensors, other dtypes, empty batches or candidate sets) evaluates
the same formulas with torch ops, so the classes work wherever the reference's do.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from pinsage_hip import loss as hl

_DIAGONAL = -1e9          # what the reference's batch-hard loss puts on the diagonal


def _hinge_mean(margin, neg_sim, pos_sim):
    return torch.relu(margin + neg_sim - pos_sim).mean()


def torch_max_margin(q, p, neg, margin):
    """the formulas with torch ops (what the device path is compared against)"""
    pos_sim = (q * p).sum(dim=1)
    if neg.dim() == 3:
        neg_sim = (q.unsqueeze(1) * neg).sum(dim=2).max(dim=1).values
    else:
        neg_sim = (q * neg).sum(dim=1)
    return _hinge_mean(margin, neg_sim, pos_sim)


def torch_batch_hard(q, p, margin):
    sim = q @ p.t()
    eye = torch.eye(q.size(0), device=q.device, dtype=torch.bool)
    neg_sim = sim.masked_fill(eye, _DIAGONAL).max(dim=1).values
    return _hinge_mean(margin, neg_sim, (q * p).sum(dim=1))


def _on_device(*tensors):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _shared_alias(neg):
    """the [N, D] tensor behind a batch-expanded [B, N, D] view, as a differentiable alias of the view's base -- or None"""
    if neg.dim() != 3 or neg.size(0) < 2 or neg.stride(0) != 0:
        return None
    base = neg._base
    if base is None:
        return None
    size, stride, offset = tuple(neg.shape[1:]), tuple(neg.stride()[1:]), neg.storage_offset()
    if tuple(base.shape) == size and tuple(base.stride()) == stride and base.storage_offset() == offset:
        return base
    try:
        return torch.as_strided(base, size, stride, offset)
    except RuntimeError:
        return None


class MaxMarginRankingLoss(nn.Module):
    def __init__(self, margin=0.1):
        super().__init__()
        self.margin = margin

    def forward(self, query_embeddings, positive_embeddings, negative_embeddings):
        q, p, neg = query_embeddings, positive_embeddings, negative_embeddings
        device = (_on_device(q, p, neg) and q.dim() == 2 and p.shape == q.shape and q.size(0) > 0 and neg.numel() > 0
                  and neg.size(0) == q.size(0) and neg.size(-1) == q.size(1) and neg.dim() in (2, 3))
        if not device:
            return torch_max_margin(q, p, neg, self.margin)
        if neg.dim() == 2:
            return hl.max_margin_per_query(q, p, neg.unsqueeze(1), self.margin)
        shared = _shared_alias(neg)
        if shared is not None:
            return hl.max_margin_shared(q, p, shared, self.margin)
        return hl.max_margin_per_query(q, p, neg, self.margin)


class BatchHardTripletLoss(nn.Module):
    def __init__(self, margin=0.1):
        super().__init__()
        self.margin = margin

    def forward(self, query_embeddings, positive_embeddings):
        q, p = query_embeddings, positive_embeddings
        if _on_device(q, p) and q.dim() == 2 and p.shape == q.shape and q.size(0) > 0:
            return hl.batch_hard(q, p, self.margin)
        return torch_batch_hard(q, p, self.margin)


class CurriculumLoss(nn.Module):
    def __init__(self, margin=0.1, epoch=0, max_epochs=10, hard_negative_factor=2.0):
        super().__init__()
        self.margin = margin
        self.epoch = epoch
        self.max_epochs = max_epochs
        self.hard_negative_factor = hard_negative_factor
        self.base_loss = MaxMarginRankingLoss(margin)

    def update_epoch(self, epoch):
        self.epoch = epoch

    def forward(self, query_embeddings, positive_embeddings, random_negative_embeddings, hard_negative_embeddings=None):
        base = self.base_loss(query_embeddings, positive_embeddings, random_negative_embeddings)
        if self.epoch < 1 or hard_negative_embeddings is None:
            return base
        hard = self.base_loss(query_embeddings, positive_embeddings, hard_negative_embeddings)
        weight = min(self.epoch, self.max_epochs) / self.max_epochs * self.hard_negative_factor
        return base + weight * hard
