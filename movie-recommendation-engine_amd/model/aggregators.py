"""model.aggregators -- drop-in for the reference module of the same name (reference
model/aggregators.py).  Same five classes, constructor arguments, parameter names and forward
signatures.  The gather + weighted reduce of Mean / Weighted / Importance aggregators runs on
ps_importance_pool (one kernel for the whole batch instead of a python loop per node);
ImportanceAggregator's Linear runs once on the pooled rows (sum_i w_i (W x_i + b) = W sum_i w_i x_i + b
because the weights sum to 1), on the fp32-MFMA kernel.  AttentionAggregator and MaxPoolingAggregator run on
ps_attention_weights + ps_importance_pool and ps_linear + ps_gather_max for CUDA fp32 inputs (no [B, T, C] tensor is ever
built); under autograd the linears are F.linear on the tape and the gather stage is sampling.attention / sampling.max_pool, whose
backward is the transposed gathers of csrc/neigh_agg_bwd.hip (sampling.grad_method = "torch" restores the torch code there).
CPU tensors and other dtypes keep the batched torch code (`_forward_torch`).
ImportanceAggregator's Linear and LayerNorm behind the pooling are a switch: `ImportanceAggregator.norm_method = "hip"` (class or
instance; the default is "torch") runs dense.linear and dense.layer_norm -- ps_layer_norm, with the rows without neighbours as its
mask -- in both directions.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from pinsage_hip import dense, sampling
from pinsage_hip import native as nv


def _pad(neighbors, n_rows, weights=None, mode="weighted"):
    """python list-of-lists -> padded numpy (ids int32[B,T], w fp32[B,T], nvalid int32[B]).
    No range filtering here (the reference indexes features[node_neighbors] directly: out-of-range
    ids raise IndexError)."""
    B = len(neighbors)
    T = max(1, max((len(r) for r in neighbors), default=1))
    ids = np.full((B, T), -1, dtype=np.int32)
    w = np.zeros((B, T), dtype=np.float32)
    nvalid = np.zeros(B, dtype=np.int32)
    for i, nb in enumerate(neighbors):
        k = len(nb)
        if k == 0:
            continue
        a = np.asarray([int(v) for v in nb], dtype=np.int64)
        if a.max() >= n_rows or a.min() < -n_rows:
            raise IndexError(f"index {int(a.max() if a.max() >= n_rows else a.min())} is out of bounds for "
                             f"dimension 0 with size {n_rows}")
        a = np.where(a < 0, a + n_rows, a)
        ids[i, :k] = a
        nvalid[i] = k
        if mode == "mean" or weights is None:
            w[i, :k] = np.float32(1.0) / np.float32(k)
        else:
            nw = [float(v) for v in list(weights[i])[:k]]            # node_weights[:len(node_neighbors)]
            if len(nw) != k:
                raise RuntimeError(f"The size of tensor a ({k}) must match the size of tensor b ({len(nw)}) "
                                   "at non-singleton dimension 0")
            s = sum(nw)
            if s == 0:
                w[i, :k] = np.float32(1.0) / np.float32(k)           # all-zero weights -> mean (:78-80,:265-267)
            else:
                w[i, :k] = np.asarray([v / s for v in nw], dtype=np.float64).astype(np.float32)
    return ids, w, nvalid


def _pool(features, ids, w, nvalid):
    dev = nv.require_gpu()
    f = (features if features.is_cuda else features.to(dev)).float().contiguous()
    # sampling.pool keeps the result on the autograd tape when `features` needs a gradient (the reference's
    # aggregators are plain differentiable torch code, model/aggregators.py:13-91,233-287)
    return sampling.pool(f, ids=torch.from_numpy(ids).to(f.device), wts=torch.from_numpy(w).to(f.device),
                         nvalid=torch.from_numpy(nvalid).to(f.device), renorm=False)


class MeanAggregator(nn.Module):
    """reference model/aggregators.py:5-39"""

    def __init__(self):
        super().__init__()

    def forward(self, features, neighbors):
        ids, w, nvalid = _pad(neighbors, int(features.size(0)), mode="mean")
        out = _pool(features, ids, w, nvalid)
        return out if features.is_cuda else out.to(features.device)


class WeightedAggregator(nn.Module):
    """reference model/aggregators.py:41-91"""

    def __init__(self):
        super().__init__()

    def forward(self, features, neighbors, weights):
        ids, w, nvalid = _pad(neighbors, int(features.size(0)), weights)
        out = _pool(features, ids, w, nvalid)
        return out if features.is_cuda else out.to(features.device)


def _pad_dev(neighbors, features):
    """_pad's ids / nvalid on the device of `features`"""
    ids, _, nvalid = _pad(neighbors, int(features.size(0)), mode="mean")
    return torch.from_numpy(ids).to(features.device), torch.from_numpy(nvalid).to(features.device)


def _off_tape(module, *tensors):
    """may the call bypass autograd?  (ImportanceAggregator.forward's test, extended to the feature tensors)"""
    return not (torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or
                                             any(p.requires_grad for p in module.parameters())))


def _cuda_fp32(t):
    return t.is_cuda and t.dtype == torch.float32


def _hip_grad(module):
    """does a call on the autograd tape take the HIP backward?  (sampling.grad_method, fp32 parameters)"""
    return sampling.grad_method == "hip" and all(p.dtype == torch.float32 for p in module.parameters())


class AttentionAggregator(nn.Module):
    """reference model/aggregators.py:93-160.  HIP path: the first attention layer split by columns -- u = self W1[:, :C]^T + b1
    over the B target rows and v = features W1[:, C:]^T over all rows, two ps_linear calls -- then ps_attention_weights
    (scores + softmax over a gather of T rows of v) and ps_importance_pool with those weights (a gather of T rows of features).
    The second layer's bias shifts all scores of a row alike and drops out of the softmax."""

    def __init__(self, in_channels):
        super().__init__()
        self.attention = nn.Sequential(nn.Linear(in_channels * 2, in_channels), nn.ReLU(), nn.Linear(in_channels, 1))

    def forward(self, features, neighbors, self_features=None):
        sf = features if self_features is None else self_features
        off_tape = _off_tape(self, features, sf)
        if not (_cuda_fp32(features) and _cuda_fp32(sf) and (off_tape or _hip_grad(self))) or features.dim() != 2 \
                or sf.dim() != 2 or sf.size(0) < len(neighbors) or sf.size(1) != features.size(1) \
                or self.attention[0].in_features != 2 * features.size(1):
            return self._forward_torch(features, neighbors, self_features)       # malformed calls raise what they always raised
        if off_tape:
            return self._hip_padded(features, *_pad_dev(neighbors, features), sf)
        return self._hip_tape(features, *_pad_dev(neighbors, features), sf)

    def _hip_tape(self, features, ids, nvalid, self_features):
        """the HIP path on the autograd tape: the two halves of the first layer are F.linear (torch supplies their gradients),
        the gather stage is sampling.attention, whose backward is csrc/neigh_agg_bwd.hip"""
        dev, C, B = features.device, int(features.size(1)), int(ids.size(0))
        W1, b1 = self.attention[0].weight.to(dev), self.attention[0].bias.to(dev)
        u = F.linear(self_features[:B], W1[:, :C], b1)
        v = F.linear(features, W1[:, C:])
        return sampling.attention(features, u, v, self.attention[2].weight.to(dev).reshape(-1), self.attention[2].bias.to(dev),
                                  ids, nvalid)

    def _hip_padded(self, features, ids, nvalid, self_features):
        """the HIP path over padded device tensors (ids int32 [B,T], nvalid int32 [B])"""
        dev, C, B = features.device, int(features.size(1)), int(ids.size(0))
        W1, b1 = self.attention[0].weight.detach().to(dev), self.attention[0].bias.detach().to(dev)
        w2 = self.attention[2].weight.detach().to(dev).reshape(-1)
        with torch.no_grad():
            u = dense.linear(self_features[:B], W1[:, :C], b1)
            v = dense.linear(features, W1[:, C:])
            return sampling.attention_pool(features, u, v, w2, ids, nvalid)

    def _forward_torch(self, features, neighbors, self_features=None):
        """batched over a padded neighbour tensor (CPU tensors, other dtypes, training)"""
        return self._torch_padded(features, *_pad_dev(neighbors, features), features if self_features is None else self_features)

    def _torch_padded(self, features, ids, nvalid, self_features):
        dev = features.device
        idt = ids.long().clamp(min=0)
        mask = torch.arange(ids.shape[1], device=dev)[None, :] < nvalid[:, None]
        nbr = features[idt]                                               # [B,T,C]
        B = idt.size(0)
        selfe = self_features[:B].unsqueeze(1).expand(-1, idt.size(1), -1)
        scores = self.attention(torch.cat([selfe, nbr], dim=2)).squeeze(2)
        scores = scores.masked_fill(~mask, float("-inf"))
        has = mask.any(dim=1, keepdim=True)
        scores = torch.where(has, scores, torch.zeros_like(scores))       # avoid NaN softmax on empty rows
        attn = torch.softmax(scores, dim=1)
        attn = torch.where(mask, attn, torch.zeros_like(attn))            # rows without neighbours -> zeros
        return (nbr * attn.unsqueeze(2)).sum(dim=1)


class MaxPoolingAggregator(nn.Module):
    """reference model/aggregators.py:162-211.  HIP path: the MLP once over all rows (ps_linear with its ReLU epilogue), then
    ps_gather_max over the neighbour lists."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(in_channels, out_channels), nn.ReLU())

    def forward(self, features, neighbors):
        off_tape = _off_tape(self, features)
        if not (_cuda_fp32(features) and (off_tape or _hip_grad(self))) or features.dim() != 2 \
                or features.size(1) != self.mlp[0].in_features:
            return self._forward_torch(features, neighbors)
        if off_tape:
            return self._hip_padded(features, *_pad_dev(neighbors, features))
        return self._hip_tape(features, *_pad_dev(neighbors, features))

    def _hip_tape(self, features, ids, nvalid):
        """the HIP path on the autograd tape: the MLP is F.linear + relu over all rows (torch supplies its gradients), the gather
        stage is sampling.max_pool, whose backward is csrc/neigh_agg_bwd.hip"""
        dev = features.device
        t = F.relu(F.linear(features, self.mlp[0].weight.to(dev), self.mlp[0].bias.to(dev)))
        return sampling.max_pool(t, ids, nvalid)

    def _hip_padded(self, features, ids, nvalid):
        """the HIP path over padded device tensors (ids int32 [B,T], nvalid int32 [B])"""
        dev = features.device
        with torch.no_grad():
            t = dense.linear(features, self.mlp[0].weight.detach().to(dev), self.mlp[0].bias.detach().to(dev), relu=True)
            return sampling.gather_max(t, ids, nvalid)

    def _forward_torch(self, features, neighbors):
        """mlp applied once per node, masked max (CPU tensors, other dtypes, training)"""
        return self._torch_padded(features, *_pad_dev(neighbors, features))

    def _torch_padded(self, features, ids, nvalid):
        dev = features.device
        idt = ids.long().clamp(min=0)
        mask = torch.arange(ids.shape[1], device=dev)[None, :] < nvalid[:, None]
        t = self.mlp(features)[idt]
        t = t.masked_fill(~mask.unsqueeze(2), float("-inf"))
        out = t.max(dim=1).values
        return torch.where(mask.any(dim=1, keepdim=True), out, torch.zeros_like(out))


class ImportanceAggregator(nn.Module):
    """reference model/aggregators.py:213-287: LayerNorm(sum_i w_i (W x_i + b)); zeros for empty rows."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.transform = nn.Linear(in_channels, out_channels)
        self.norm = nn.LayerNorm(out_channels)

    # how the Linear and the LayerNorm behind the pooling are computed: "torch" (the default) keeps F.linear on the tape and
    # F.layer_norm + torch.where in both directions; "hip" runs dense.linear and dense.layer_norm (ps_layer_norm with the rows
    # without neighbours as its `live` mask; on the tape, under sampling.grad_method == "hip", their HIP backwards).  Set on the
    # class or on an instance.
    norm_method = "torch"

    def _hip_norm(self, features):
        """does this call take the kernel path?"""
        if self.norm_method not in ("hip", "torch"):
            raise ValueError(f"ImportanceAggregator.norm_method must be 'hip' or 'torch', not {self.norm_method!r}")
        n = self.norm
        return (self.norm_method == "hip" and _cuda_fp32(features) and features.dim() == 2 and type(n) is nn.LayerNorm
                and n.elementwise_affine and n.bias is not None and tuple(n.normalized_shape) == (self.transform.out_features,)
                and all(p.dtype == torch.float32 and p.device == features.device for p in self.parameters()))

    def forward(self, features, neighbors, importance_weights):
        hip = self._hip_norm(features)
        ids, w, nvalid = _pad(neighbors, int(features.size(0)), importance_weights)
        pooled = _pool(features, ids, w, nvalid)
        if hip:
            # dense.linear and dense.layer_norm route themselves: off the tape one kernel each, on it LinearFn / LayerNormFn
            t = dense.linear(pooled, self.transform.weight, self.transform.bias)
            return dense.layer_norm(t, self.norm.weight, self.norm.bias, self.norm.eps,
                                    live=torch.from_numpy(nvalid).to(t.device))
        if torch.is_grad_enabled() and (pooled.requires_grad or any(p.requires_grad for p in self.parameters())):
            t = F.linear(pooled, self.transform.weight.to(pooled.device), self.transform.bias.to(pooled.device))
        else:
            t = dense.linear(pooled, self.transform.weight.detach().to(pooled.device),
                             self.transform.bias.detach().to(pooled.device))
        normed = F.layer_norm(t, self.norm.normalized_shape, self.norm.weight.to(t.device), self.norm.bias.to(t.device),
                              self.norm.eps)
        has = torch.from_numpy(nvalid > 0).to(t.device).unsqueeze(1)
        out = torch.where(has, normed, torch.zeros_like(normed))
        return out if features.is_cuda else out.to(features.device)
