"""model.layers -- drop-in for the reference module of the same name (reference model/layers.py).  Same four classes,
constructor arguments, attribute names, initialisation and forward signatures; a reference state_dict loads unchanged.

GraphConvLayer on CUDA fp32 inputs outside autograd: the three linear maps are composed per call (as shard.fused_self_update does
for PinSage) and run as ONE ps_linear over [x | neigh_x] -- the torch.cat never exists -- followed, in training mode, by
ps_bn_batch_stats (column mean / biased variance from fp64 sums, running statistics updated in place) and ps_bn_apply in place
(normalise, ReLU, F.normalize).  In eval mode batch norm is a per-column affine map and is folded into the composed weights: the
layer is one ps_linear launch with its ReLU + L2 epilogue.  The three pooling layers pad their python lists once on the host
(with the reference's filtering and weight quirks, see _pad) and run on ps_importance_pool / ps_gather_max.  CPU tensors, other
dtypes, calls that autograd has to see and a batch norm that is not the default configuration run the torch code
(`_forward_torch`).

Training on the kernels is a switch: `GraphConvLayer.grad_method = "hip"` (class or instance; the default is "torch") together with
sampling.grad_method == "hip" keeps a training-mode call with gradients on the tape as a differentiable dense.linear over the
composed weights and dense.batch_norm, whose backward is ps_bn_bwd (`_forward_hip_tape`: same output and buffer bits as off the
tape).  Eval mode with gradients (M >= 2), an empty batch and a non-default batch norm run `_forward_torch` under either setting."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from pinsage_hip import dense, sampling


def _cuda_fp32(t):
    return t.is_cuda and t.dtype == torch.float32


def _off_tape(module, *tensors):
    """may the call bypass autograd?  (model/aggregators.py's test)"""
    return not (torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or
                                             any(p.requires_grad for p in module.parameters())))


class GraphConvLayer(nn.Module):
    """reference model/layers.py:5-77: normalize(relu(bn(linear_out(cat[linear_self(x), linear_neigh(neigh_x)])))), the batch
    norm skipped for a single row."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.linear_self = nn.Linear(in_channels, out_channels)
        self.linear_neigh = nn.Linear(in_channels, out_channels)
        self.linear_out = nn.Linear(2 * out_channels, out_channels)
        self.bn = nn.BatchNorm1d(out_channels)
        self._init_weights()

    def _init_weights(self):
        nn.init.xavier_uniform_(self.linear_self.weight)
        nn.init.xavier_uniform_(self.linear_neigh.weight)
        nn.init.xavier_uniform_(self.linear_out.weight)
        nn.init.zeros_(self.linear_self.bias)
        nn.init.zeros_(self.linear_neigh.bias)
        nn.init.zeros_(self.linear_out.bias)

    # how a call that autograd has to see is computed: "torch" (the default) runs `_forward_torch`; "hip" -- together with
    # sampling.grad_method == "hip" -- keeps the kernels on the tape (`_forward_hip_tape`).  Set on the class or on an instance.
    grad_method = "torch"

    def forward(self, x, neigh_x):
        if self.grad_method not in ("hip", "torch"):
            raise ValueError(f"GraphConvLayer.grad_method must be 'hip' or 'torch', not {self.grad_method!r}")
        if self._hip_shapes(x, neigh_x):
            if _off_tape(self, x, neigh_x):
                return self._forward_hip(x, neigh_x)
            M = x.size(0)
            if self.grad_method == "hip" and sampling.grad_method == "hip" and (M == 1 or (M >= 2 and self.bn.training)):
                return self._forward_hip_tape(x, neigh_x)
        return self._forward_torch(x, neigh_x)

    def _hip_serves(self, x, neigh_x):
        """do the kernels serve the call off the tape?"""
        return self._hip_shapes(x, neigh_x) and _off_tape(self, x, neigh_x)

    def _hip_shapes(self, x, neigh_x):
        """the shape / dtype / device / batch-norm-configuration conditions of the kernels, on or off the tape"""
        bn = self.bn
        if not (_cuda_fp32(x) and _cuda_fp32(neigh_x) and x.dim() == 2 and neigh_x.dim() == 2):
            return False
        if x.size(0) != neigh_x.size(0) or x.size(1) != self.linear_self.in_features \
                or neigh_x.size(1) != self.linear_neigh.in_features or x.device != neigh_x.device:
            return False                                                  # malformed calls raise what the torch code raises
        if not (type(bn) is nn.BatchNorm1d and bn.affine and bn.track_running_stats and bn.momentum is not None):
            return False
        return all(t.device == x.device and t.dtype == torch.float32 for t in list(self.parameters()) + list(self.buffers())
                   if t is not bn.num_batches_tracked)

    def _composed(self, s=None, shift=None, tape=False):
        """(W1, W2, b) with linear_out(cat[linear_self(x), linear_neigh(n)]) = x W1^T + n W2^T + b: W1 = Wo[:, :O] Ws,
        W2 = Wo[:, O:] Wn, b = Wo[:, :O] bs + Wo[:, O:] bn + bo (three small GEMMs on the weights instead of two [M, O]
        intermediates).  With s / shift (fp32 [O]; off the tape only) the per-column affine map t -> s t + shift is folded in: the
        rows of Wo are scaled before the products and b becomes Wo'[:, :O] bs + Wo'[:, O:] bn + (s bo + shift).  The two halves
        of Wo are made contiguous (and scaled) in one launch.  Nothing is cached: see shard.fused_self_update.
        tape=True: over the six leaves themselves, so that the three dense.linear calls and the copy of Wo's halves stay on the
        autograd tape and carry dW1, dW2, db back to them -- the same calls, hence the same bits."""
        params = (self.linear_self.weight, self.linear_self.bias, self.linear_neigh.weight, self.linear_neigh.bias,
                  self.linear_out.weight, self.linear_out.bias)
        Ws, bs, Wn, bn_, Wo, bo = params if tape else (p.detach() for p in params)
        O = Ws.size(0)
        halves = Wo.view(O, 2, O).permute(1, 0, 2)                        # [2, O, O]: Wo[:, :O], Wo[:, O:]
        if s is None:
            Wo12 = halves.contiguous()
        else:
            Wo12 = torch.empty((2, O, O), dtype=Wo.dtype, device=Wo.device)
            torch.mul(halves, s[None, :, None], out=Wo12)
            bo = torch.addcmul(shift, s, bo)
        W1 = dense.linear(Wo12[0], Ws.t())                                # dense.linear makes the transposed weight contiguous
        W2 = dense.linear(Wo12[1], Wn.t())
        b = dense.linear(bs.reshape(1, -1), Wo12[0], bo, x2=bn_.reshape(1, -1), W2=Wo12[1]).reshape(-1)
        return W1, W2, b

    def _forward_hip(self, x, neigh_x):
        bn = self.bn
        M = x.size(0)
        with torch.no_grad():
            if M == 0:
                return x.new_empty((0, self.linear_out.out_features))
            gamma, beta = bn.weight.detach(), bn.bias.detach()
            if M == 1 or not bn.training:
                if M == 1:                                                # no batch norm, the buffers stay as they are
                    W1, W2, b = self._composed()
                else:
                    # eval: bn(t) = s t + (beta - s rm) with s = gamma / sqrt(rv + eps), folded into the composed map
                    s = gamma / torch.sqrt(bn.running_var + bn.eps)
                    W1, W2, b = self._composed(s, torch.addcmul(beta, s, bn.running_mean, value=-1.0))
                return dense.linear(x, W1, b, x2=neigh_x, W2=W2, relu=True, l2norm=True)
            W1, W2, b = self._composed()
            z = dense.linear(x, W1, b, x2=neigh_x, W2=W2)
            mean, _, scale = dense.batch_norm_stats(z, gamma, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
            bn.num_batches_tracked.add_(1)
            return dense.batch_norm_apply(z, mean, scale, beta, relu=True, l2norm=True, out=z)

    def _forward_hip_tape(self, x, neigh_x):
        """grad_method "hip", a call autograd has to see: training mode with M >= 2 -- one differentiable dense.linear over
        [x | neigh_x] with the composed weights, then dense.batch_norm (ps_bn_batch_stats + ps_bn_apply forward, ps_bn_bwd
        backward; z is the only [M, O] tensor saved) -- and M == 1 in either mode (no batch norm, the buffers untouched).  The
        output and the buffers have the bits of `_forward_hip`.  Eval mode with M >= 2, M == 0 and a non-default batch norm stay
        with `_forward_torch`."""
        bn = self.bn
        W1, W2, b = self._composed(tape=True)
        if x.size(0) == 1:
            return dense.linear(x, W1, b, x2=neigh_x, W2=W2, relu=True, l2norm=True)
        z = dense.linear(x, W1, b, x2=neigh_x, W2=W2)
        y = dense.batch_norm(z, bn.weight, bn.bias, bn.eps, bn.momentum, bn.running_mean, bn.running_var, relu=True, l2norm=True)
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
        return y

    def _forward_torch(self, x, neigh_x):
        """the reference's forward in torch (CPU tensors, other dtypes, calls on the tape unless grad_method is "hip", a
        non-default bn); the concatenation is replaced by the two column halves of linear_out"""
        O = self.linear_self.out_features
        Wo = self.linear_out.weight
        out = F.linear(self.linear_self(x), Wo[:, :O]) + F.linear(self.linear_neigh(neigh_x), Wo[:, O:], self.linear_out.bias)
        if out.size(0) > 1:
            out = self.bn(out)
        return F.normalize(F.relu(out), p=2, dim=1)


def _pad(neighbors, weights, n_rows, mode):
    """python list-of-lists -> padded numpy (ids int32 [B,T], w fp32 [B,T] or None, nvalid int32 [B]) with the quirks of the
    reference's loops (model/layers.py:102-131, 158-193, 218-235):
      * an id is kept iff id < n_rows; a negative id indexes from the end; an id below -n_rows raises IndexError
      * the weights of a row are weights[i][:len(kept)] -- the FIRST len(kept) weights, whatever positions were kept --
        normalised by python's left-to-right sum() in float64, then rounded to fp32
      * a zero sum: uniform weights fp32(1 / len) (mode "importance") or the mean (mode "wmean")
      * mode "wmean": weights None, or no weights[i], is the mean; mode "importance": zip() stops at the shorter list
      * mode "max": no weights
    A row that is empty, or filtered to nothing, has nvalid 0 (a zero output row)."""
    if mode == "importance":
        neighbors = neighbors[:len(weights)] if len(weights) < len(neighbors) else neighbors
    B = len(neighbors)
    kept_rows = []
    for nb in neighbors:
        kept = [int(n) for n in nb if n < n_rows] if nb else []
        for n in kept:
            if n < -n_rows:
                raise IndexError(f"index {n} is out of bounds for dimension 0 with size {n_rows}")
        kept_rows.append([n + n_rows if n < 0 else n for n in kept])
    T = max(1, max((len(r) for r in kept_rows), default=1))
    ids = np.full((B, T), -1, dtype=np.int32)
    nvalid = np.zeros(B, dtype=np.int32)
    w = None if mode == "max" else np.zeros((B, T), dtype=np.float32)
    for i, kept in enumerate(kept_rows):
        k = len(kept)
        if k == 0:
            continue
        ids[i, :k] = kept
        nvalid[i] = k
        if mode == "max":
            continue
        if mode == "wmean" and (weights is None or len(weights) <= i):
            w[i, :k] = np.float32(1.0) / np.float32(k)
            continue
        nw = list(weights[i][:k])
        s = sum(nw)
        if s == 0:
            w[i, :k] = np.float32(1.0 / k) if mode == "importance" else np.float32(1.0) / np.float32(k)
            continue
        nw = np.asarray([v / s for v in nw], dtype=np.float64).astype(np.float32)
        if len(nw) != k and len(nw) != 1:                                 # a single weight broadcasts over the rows, as in torch
            raise RuntimeError(f"The size of tensor a ({k}) must match the size of tensor b ({len(nw)}) "
                               "at non-singleton dimension 0")
        w[i, :k] = nw
    return ids, w, nvalid


def _no_rows():
    return torch.stack([])                                               # raises what the reference's torch.stack(pooled_list) raises


class _ListPooling(nn.Module):
    """the three pooling layers: pad on the host, one kernel over the batch"""
    _mode = ""

    def __init__(self):
        super().__init__()

    def _run(self, x, neighbors, weights):
        if len(neighbors) == 0 or (self._mode == "importance" and len(weights) == 0):
            return _no_rows()
        ids, w, nvalid = _pad(neighbors, weights, int(x.size(0)), self._mode)
        dev = x.device
        ids_t, nvalid_t = torch.from_numpy(ids).to(dev), torch.from_numpy(nvalid).to(dev)
        w_t = torch.from_numpy(w).to(dev) if w is not None else None
        # sampling.pool / sampling.max_pool keep their result on the autograd tape when x needs a gradient; with
        # sampling.grad_method = "torch" the maximum under autograd is the torch code below
        if _cuda_fp32(x) and x.dim() == 2 and not (self._mode == "max" and torch.is_grad_enabled() and x.requires_grad
                                                   and sampling.grad_method != "hip"):
            return self._hip_padded(x, ids_t, w_t, nvalid_t)
        return self._torch_padded(x, ids_t, w_t, nvalid_t)

    def _forward_torch(self, x, neighbors, weights=None):
        """batched torch code over the padded lists (CPU tensors, other dtypes, features on the autograd tape)"""
        if len(neighbors) == 0 or (self._mode == "importance" and len(weights) == 0):
            return _no_rows()
        ids, w, nvalid = _pad(neighbors, weights, int(x.size(0)), self._mode)
        dev = x.device
        return self._torch_padded(x, torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev) if w is not None else None,
                                  torch.from_numpy(nvalid).to(dev))

    def _hip_padded(self, x, ids, w, nvalid):
        return sampling.pool(x, ids=ids, wts=w, nvalid=nvalid, renorm=False)

    def _torch_padded(self, x, ids, w, nvalid):
        nbr = x[ids.long().clamp(min=0)]                                  # [B,T,...]; the padding carries weight 0
        return (nbr * w.to(x.dtype).reshape(w.shape + (1,) * (x.dim() - 1))).sum(dim=1)


class ImportancePoolingLayer(_ListPooling):
    """reference model/layers.py:79-133"""
    _mode = "importance"

    def forward(self, x, neighbors, weights):
        return self._run(x, neighbors, weights)


class WeightedMeanPoolingLayer(_ListPooling):
    """reference model/layers.py:135-195"""
    _mode = "wmean"

    def forward(self, x, neighbors, weights=None):
        return self._run(x, neighbors, weights)


class MaxPoolingLayer(_ListPooling):
    """reference model/layers.py:197-237"""
    _mode = "max"

    def forward(self, x, neighbors):
        return self._run(x, neighbors, None)

    def _forward_torch(self, x, neighbors):
        return super()._forward_torch(x, neighbors, None)

    def _hip_padded(self, x, ids, w, nvalid):
        return sampling.max_pool(x, ids, nvalid)

    def _torch_padded(self, x, ids, w, nvalid):
        mask = torch.arange(ids.shape[1], device=x.device)[None, :] < nvalid[:, None]
        t = x[ids.long().clamp(min=0)]
        t = t.masked_fill(~mask.reshape(mask.shape + (1,) * (x.dim() - 1)), float("-inf"))
        out = t.max(dim=1).values
        return torch.where(mask.any(dim=1).reshape((-1,) + (1,) * (x.dim() - 1)), out, torch.zeros_like(out))
