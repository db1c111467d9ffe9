"""Dense / retrieval ops over libpinsage_hip.so: fp32-MFMA linear layers with fused epilogues,
LSH encode (projection + ballot bit-pack), Hamming top-k, exact dot top-k."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import native as nv


def _rowmajor(w):
    """(tensor to keep alive, leading dimension) for a 2-D fp32 matrix whose rows are contiguous
    (column slices of a row-major weight are fine: no copy, ld = stride(0))."""
    if w.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if w.dim() != 2:
        raise ValueError("2-D matrix expected")
    if w.stride(1) != 1 or w.stride(0) < w.size(1):
        w = w.contiguous()
    return w, w.stride(0) if w.size(0) > 1 else max(w.stride(0), w.size(1))


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise nv.NativeError("libpinsage_hip takes device (HBM) tensors; got a CPU tensor (no CPU fallback)")


class StagedWeight:
    """A weight matrix stored in the order the GEMM kernel stages it (ps_permute_k: every group of eight k as
    0 2 4 6 1 3 5 7).  linear() / lsh_encode() take it in place of the plain matrix (PS_WPERM): same results bit for bit,
    32 fewer vector instructions per 64 MFMAs.  For matrices that are multiplied many times (model weights, LSH rotation)."""
    __slots__ = ("t", "shape")

    def __init__(self, t):
        self.t = t
        self.shape = t.shape

    def size(self, i):
        return self.t.size(i)


def stage_weight(W):
    """StagedWeight of a [N, K] device matrix, or W itself when the kernel's staged path does not apply (K % 32 != 0)."""
    if isinstance(W, StagedWeight) or W is None:
        return W
    _require_cuda(W)
    if W.dim() != 2 or W.dtype != torch.float32 or W.size(1) % 32 != 0:
        return W
    Wk, ld = _rowmajor(W)
    out = torch.empty((Wk.size(0), Wk.size(1)), dtype=torch.float32, device=W.device)
    with torch.cuda.device(W.device):
        nv.call("ps_permute_k", nv.ptr(Wk, contiguous=False), Wk.size(0), Wk.size(1), ld, nv.ptr(out), nv.stream())
    return StagedWeight(out)


class StagedLsh:
    """An LSH rotation as ps_lsh_stage stores it (the fp32 matrix, its bf16 hi + lo split in MFMA operand order, a bound of
    every row norm).  lsh_encode() takes it in place of the matrix (PS_LSH_STAGED): the same codes bit for bit, the signs
    decided on the bf16 matrix pipe wherever that is beyond doubt and by the exact fmaf chain elsewhere (csrc/lsh_filter.hip).
    `image` is the uint8 device buffer; stats() reads its two counters (they move under PS_LSH_STATS=1 only)."""
    __slots__ = ("image", "shape")

    def __init__(self, image, nbits, d):
        self.image = image
        self.shape = (nbits, d)

    def size(self, i):
        return self.shape[i]

    def stats(self):
        """(dots decided, dots that took the exact chain) since the image was staged"""
        seen, flagged = self.image[16:32].view(torch.int64).tolist()
        return seen, flagged


def stage_lsh(A):
    """StagedLsh of a [nbits, d] device rotation; where ps_lsh_stage does not serve the shape, and under PS_LSH_FILTER=0,
    stage_weight(A) (the fp32 kernels)."""
    if isinstance(A, (StagedLsh, StagedWeight)) or A is None:
        return A
    _require_cuda(A)
    if os.environ.get("PS_LSH_FILTER", "1") == "0" or A.dim() != 2 or A.dtype != torch.float32:
        return stage_weight(A)
    nbits, d = A.size(0), A.size(1)
    nbytes = nv.lib().ps_lsh_stage_bytes(nbits, d)
    if nbytes == 0:
        return stage_weight(A)
    Ak = A.contiguous()
    image = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
    with torch.cuda.device(A.device):
        nv.call("ps_lsh_stage", nv.ptr(Ak), nbits, d, nv.ptr(image), nbytes, nv.stream())
    return StagedLsh(image, nbits, d)


def linear(x, W, b=None, x2=None, W2=None, relu=False, l2norm=False):
    """y = epi(x @ W.T (+ x2 @ W2.T) + b): nn.Linear / F.relu / torch.cat / F.normalize of
    PinSage.forward (reference model/pinsage.py:202,235-240,248-249) in one kernel.  W / W2: matrices or StagedWeights (both
    or neither).
    With autograd on and an operand that requires a gradient the call stays on the tape: LinearFn (the same kernel forward,
    ps_linear_epilogue_bwd / ps_linear_wgrad / ps_linear backward) for CUDA fp32 operands under sampling.grad_method == "hip",
    linear_torch elsewhere ("torch", other dtypes, CPU tensors; a backward that is itself to be differentiated needs "torch" too:
    LinearFn is once-differentiable).  StagedWeights are derived copies, not leaves: ValueError there."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, W, b, x2, W2)):
        if isinstance(W, StagedWeight) or isinstance(W2, StagedWeight):
            raise ValueError("a StagedWeight is a derived copy, not a leaf: pass the weight itself where a gradient is needed")
        from .graph import use_hip_grad
        if use_hip_grad(*(t for t in (x, W, b, x2, W2) if t is not None)):
            return LinearFn.apply(x, W, b, x2, W2, bool(relu), bool(l2norm))
        return linear_torch(x, W, b, x2, W2, relu, l2norm)
    return _linear_fwd(x, W, b, x2, W2, relu, l2norm)


def linear_torch(x, W, b=None, x2=None, W2=None, relu=False, l2norm=False):
    """linear() as a differentiable torch expression (grad_method "torch", other dtypes)"""
    y = F.linear(x, W, b)
    if x2 is not None:
        y = y + F.linear(x2, W2)
    if relu:
        y = F.relu(y)
    return F.normalize(y, p=2, dim=1) if l2norm else y


def _linear_fwd(x, W, b=None, x2=None, W2=None, relu=False, l2norm=False):
    """ps_linear, off the tape"""
    staged = isinstance(W, StagedWeight)
    if x2 is not None and isinstance(W2, StagedWeight) != staged:
        raise ValueError("W and W2 must both be staged or both plain")
    if staged:
        W, W2 = W.t, (W2.t if W2 is not None else None)
    _require_cuda(x, W, b, x2, W2)
    x = x.contiguous()
    if x.dtype != torch.float32:
        raise TypeError("fp32 expected")
    M, K = x.size(0), x.size(1)
    Wk, ldw = _rowmajor(W)
    N = Wk.size(0)
    if Wk.size(1) != K:
        raise ValueError(f"shape mismatch: x [{M},{K}] vs W {tuple(Wk.shape)}")
    K2, ldw2, W2k = 0, 0, None
    if x2 is not None:
        x2 = x2.contiguous()
        W2k, ldw2 = _rowmajor(W2)
        K2 = x2.size(1)
        if W2k.size(1) != K2 or W2k.size(0) != N or x2.size(0) != M:
            raise ValueError("shape mismatch in the second operand pair")
    if b is not None:
        b = b.contiguous()
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    flags = (nv.PS_RELU if relu else 0) | (nv.PS_L2NORM if l2norm else 0) | (nv.PS_WPERM if staged else 0)
    with torch.cuda.device(x.device):
        nv.call("ps_linear", nv.ptr(x), M, K, nv.ptr(Wk, contiguous=False), ldw, nv.ptr(b), N, nv.ptr(x2), K2,
                nv.ptr(W2k, contiguous=False), ldw2, flags, nv.ptr(y), nv.stream())
    return y


def linear_wgrad(g, x, bias=True):
    """(dW [N, K], db [N] or None) = (g.T @ x, g.sum(0)) of g [M, N], x [M, K] (ps_linear_wgrad): per element the fmaf chain over
    the rows of a partition of ps_linear_wgrad_partition(M) rows, the partitions added in order -- no atomics, the same bits on
    every run.  The workspace comes from torch's allocator."""
    _require_cuda(g, x)
    if g.dtype != torch.float32 or x.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if g.dim() != 2 or x.dim() != 2 or g.size(0) != x.size(0):
        raise ValueError(f"shape mismatch: g {tuple(g.shape)} vs x {tuple(x.shape)}")
    g, x = g.contiguous(), x.contiguous()
    M, N, K = g.size(0), g.size(1), x.size(1)
    dW = torch.empty((N, K), dtype=torch.float32, device=g.device)
    db = torch.empty(N, dtype=torch.float32, device=g.device) if bias else None
    ws, wsb = nv.workspace("ps_linear_wgrad_workspace_bytes", g.device, M, N, K)
    with torch.cuda.device(g.device):
        nv.call("ps_linear_wgrad", nv.ptr(g), M, N, nv.ptr(x), K, nv.ptr(dW), nv.ptr(db), nv.ptr(ws), wsb, nv.stream())
    return dW, db


def linear_epilogue_bwd(t, g, relu, l2norm, out=None):
    """The gradient of the pre-activation from the gradient g of linear()'s output and the saved activation t (after bias and
    ReLU, before the norm): ps_linear_epilogue_bwd, one wave per row.  out=g works in place."""
    _require_cuda(t, g, out)
    if t.dtype != torch.float32 or g.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if t.dim() != 2 or t.shape != g.shape:
        raise ValueError(f"shape mismatch: t {tuple(t.shape)} vs g {tuple(g.shape)}")
    t = t.contiguous()
    if out is None:
        g = g.contiguous()
        out = torch.empty_like(g)
    elif out.dtype != torch.float32 or out.shape != g.shape or not out.is_contiguous() or not g.is_contiguous() or out.device != g.device:
        raise ValueError("out must be a contiguous fp32 tensor of g's shape on its device (and g contiguous)")
    flags = (nv.PS_RELU if relu else 0) | (nv.PS_L2NORM if l2norm else 0)
    with torch.cuda.device(g.device):
        nv.call("ps_linear_epilogue_bwd", nv.ptr(t), nv.ptr(g), t.size(0), t.size(1), flags, nv.ptr(out), nv.stream())
    return out


class LinearFn(torch.autograd.Function):
    """Differentiable linear() for CUDA fp32 operands.  Forward: t = ps_linear with the bias and the ReLU and without the norm --
    the inference call's bits -- and, with l2norm, y = ps_bn_apply(t, mean 0, scale 1, beta 0, PS_L2NORM), the row norm the
    backward restates (fmaf(t - 0, 1, +0) is t).  Backward: gz = ps_linear_epilogue_bwd(t, gy); dW, db = ps_linear_wgrad(gz, x);
    dW2 = ps_linear_wgrad(gz, x2); dx = ps_linear(gz, W^T) and dx2 likewise, each only for an input that needs it.  t is kept only
    when the ReLU or the norm needs it, x / x2 only when a weight needs a gradient, W / W2 only when an input does.  No float
    atomics, nothing waits for the host: the same bits on every run."""

    @staticmethod
    def forward(ctx, x, W, b, x2, W2, relu, l2norm):
        need = ctx.needs_input_grad
        t = _linear_fwd(x, W, b, x2, W2, relu, False)
        y = t
        if l2norm:
            N = t.size(1)
            zero, one = torch.zeros(N, dtype=torch.float32, device=t.device), torch.ones(N, dtype=torch.float32, device=t.device)
            y = batch_norm_apply(t, zero, one, zero, False, True)
        ctx.relu, ctx.l2norm = relu, l2norm
        ctx.save_for_backward(x if need[1] else None, W if need[0] else None,
                              x2 if x2 is not None and need[4] else None, W2 if x2 is not None and need[3] else None,
                              t if relu or l2norm else None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, W, x2, W2, t = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = gy.contiguous()                                           # y.sum().backward() hands over a stride-0 tensor
        gz = linear_epilogue_bwd(t, g, ctx.relu, ctx.l2norm) if t is not None else g
        dx = dW = db = dx2 = dW2 = None
        if need[1]:
            dW, db = linear_wgrad(gz, x, bias=need[2])
        elif need[2]:
            # the bias gradient alone: the weight gradient against a column of ones is the same chain, acc = fmaf(g, 1, acc)
            db = linear_wgrad(gz, torch.ones((gz.size(0), 1), dtype=torch.float32, device=gz.device), bias=False)[0].view(-1)
        if need[4]:
            dW2 = linear_wgrad(gz, x2, bias=False)[0]
        if need[0]:
            dx = _linear_fwd(gz, W.t().contiguous())
        if need[3]:
            dx2 = _linear_fwd(gz, W2.t().contiguous())
        return dx, dW, db, dx2, dW2, None, None


BN_STATS_ROWS = 128       # rows per partition of ps_bn_batch_stats' fixed summation order (csrc/batch_norm.hip)


def _fp32_vec(name, t, n, device):
    if t.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if t.dim() != 1 or t.numel() != n or t.device != device:
        raise ValueError(f"{name} must be a float32 [{n}] vector on the device of z")
    return t.contiguous()


def batch_norm_stats(z, gamma, eps, momentum, running_mean=None, running_var=None):
    """(mean, var, scale) fp32 [N] of the columns of z [M, N], M >= 2 (ps_bn_batch_stats): the batch mean, the biased batch
    variance and gamma / sqrt(var + eps), from fp64 sums made in one pass over z in a fixed order -- the statistics training-mode
    nn.BatchNorm1d normalises with.  running_mean / running_var (both or neither) are updated IN PLACE as that module updates
    them: (1 - momentum) old + momentum new, the variance entering with the unbiased factor M / (M - 1)."""
    _require_cuda(z, gamma, running_mean, running_var)
    if z.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if z.dim() != 2:
        raise ValueError("2-D matrix expected")
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var: both or neither")
    z = z.contiguous()
    M, N = z.size(0), z.size(1)
    gamma = _fp32_vec("gamma", gamma, N, z.device)
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and (_fp32_vec(name, t, N, z.device) is not t or not t.is_contiguous()):
            raise ValueError(f"{name} is updated in place: it must be contiguous")
    mean, var, scale = (torch.empty(N, dtype=torch.float32, device=z.device) for _ in range(3))
    ws, wsb = nv.workspace("ps_bn_stats_workspace_bytes", z.device, M, N)
    with torch.cuda.device(z.device):
        nv.call("ps_bn_batch_stats", nv.ptr(z), M, N, nv.ptr(gamma), float(eps), float(momentum), nv.ptr(running_mean),
                nv.ptr(running_var), nv.ptr(mean), nv.ptr(var), nv.ptr(scale), nv.ptr(ws), wsb, nv.stream())
    return mean, var, scale


def batch_norm_apply(z, mean, scale, beta, relu, l2norm, out=None):
    """y = epi((z - mean) * scale + beta) per column of z [M, N] (ps_bn_apply): the normalisation of nn.BatchNorm1d with the
    F.relu / F.normalize of GraphConvLayer.forward behind it, one wave per row.  out: a contiguous fp32 [M, N] device tensor to
    write into; out=z works in place and gives the bits of a new tensor."""
    _require_cuda(z, mean, scale, beta, out)
    if z.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if z.dim() != 2:
        raise ValueError("2-D matrix expected")
    if out is None or out is not z:
        z = z.contiguous()
    elif not z.is_contiguous():
        raise ValueError("in place: z must be contiguous")
    M, N = z.size(0), z.size(1)
    mean, scale, beta = (_fp32_vec(n, t, N, z.device) for n, t in (("mean", mean), ("scale", scale), ("beta", beta)))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=z.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, N) or not out.is_contiguous() or out.device != z.device:
        raise ValueError("out must be a contiguous fp32 [M, N] tensor on the device of z")
    flags = (nv.PS_RELU if relu else 0) | (nv.PS_L2NORM if l2norm else 0)
    with torch.cuda.device(z.device):
        nv.call("ps_bn_apply", nv.ptr(z), M, N, nv.ptr(mean), nv.ptr(scale), nv.ptr(beta), flags, nv.ptr(out), nv.stream())
    return out


def batch_norm_bwd(z, gy, mean, var, scale, beta, eps, relu, l2norm, need_gz=True, need_affine=True, out=None):
    """(gz [M, N], dgamma [N], dbeta [N]) of y = epi((z - mean) * scale + beta) where mean / var / scale are batch_norm_stats' of
    this same z, M >= 2 (ps_bn_bwd): the backward of training-mode nn.BatchNorm1d with the layer's epilogue, the statistics'
    dependence on z included.  t is recomputed from z with the forward's bits; the workspace comes from torch's allocator.
    need_gz / need_affine False: that output is None and not computed.  out: a contiguous fp32 [M, N] device tensor for gz;
    out=gy works in place."""
    _require_cuda(z, gy, mean, var, scale, beta, out)
    if z.dtype != torch.float32 or gy.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if z.dim() != 2 or z.shape != gy.shape:
        raise ValueError(f"shape mismatch: z {tuple(z.shape)} vs gy {tuple(gy.shape)}")
    z = z.contiguous()
    M, N = z.size(0), z.size(1)
    if M < 2:
        raise ValueError("batch norm needs at least two rows")
    mean, var, scale, beta = (_fp32_vec(n, t, N, z.device) for n, t in (("mean", mean), ("var", var), ("scale", scale), ("beta", beta)))
    gz = dgamma = dbeta = None
    if out is None:
        gy = gy.contiguous()
        if need_gz:
            gz = torch.empty((M, N), dtype=torch.float32, device=z.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, N) or not out.is_contiguous() or not gy.is_contiguous() \
            or out.device != z.device:
        raise ValueError("out must be a contiguous fp32 [M, N] tensor on the device of z (and gy contiguous)")
    elif need_gz:
        gz = out
    if need_affine:
        dgamma, dbeta = (torch.empty(N, dtype=torch.float32, device=z.device) for _ in range(2))
    flags = (nv.PS_RELU if relu else 0) | (nv.PS_L2NORM if l2norm else 0)
    ws, wsb = nv.workspace("ps_bn_bwd_workspace_bytes", z.device, M, N)
    with torch.cuda.device(z.device):
        nv.call("ps_bn_bwd", nv.ptr(z), nv.ptr(gy), M, N, nv.ptr(mean), nv.ptr(var), nv.ptr(scale), nv.ptr(beta), float(eps), flags,
                nv.ptr(gz), nv.ptr(dgamma), nv.ptr(dbeta), nv.ptr(ws), wsb, nv.stream())
    return gz, dgamma, dbeta


def batch_norm_torch(z, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, relu=False, l2norm=False):
    """batch_norm() as a differentiable torch expression (grad_method "torch", other dtypes, CPU tensors)"""
    y = F.batch_norm(z, running_mean, running_var, gamma, beta, training=True, momentum=momentum, eps=eps)
    if relu:
        y = F.relu(y)
    return F.normalize(y, p=2, dim=1) if l2norm else y


def batch_norm(z, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, relu=False, l2norm=False):
    """Training-mode batch norm of z [M >= 2, N] with GraphConvLayer's epilogue: y = epi((z - mean) * gamma / sqrt(var + eps) +
    beta) over the batch statistics of z; running_mean / running_var (both or neither) are updated in place, once.
    Off the tape: batch_norm_stats + batch_norm_apply into a new tensor.  With autograd on and z, gamma or beta requiring a
    gradient the call stays on the tape: BatchNormFn (the same two kernels forward, ps_bn_bwd backward) for CUDA fp32 operands under
    sampling.grad_method == "hip", batch_norm_torch elsewhere ("torch", other dtypes, CPU tensors; a backward that is itself to be
    differentiated needs "torch" too: BatchNormFn is once-differentiable)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (z, gamma, beta)):
        from .graph import use_hip_grad
        if use_hip_grad(*(t for t in (z, gamma, beta, running_mean, running_var) if t is not None)):
            with torch.no_grad():
                mean, var, scale = batch_norm_stats(z, gamma, eps, momentum, running_mean, running_var)
            return BatchNormFn.apply(z, gamma, beta, mean, var, scale, float(eps), bool(relu), bool(l2norm))
        return batch_norm_torch(z, gamma, beta, eps, momentum, running_mean, running_var, relu, l2norm)
    mean, _, scale = batch_norm_stats(z, gamma, eps, momentum, running_mean, running_var)
    return batch_norm_apply(z, mean, scale, beta, relu, l2norm)


class BatchNormFn(torch.autograd.Function):
    """Differentiable batch_norm() for CUDA fp32 operands.  The statistics (mean, var, scale = gamma / sqrt(var + eps)) are made
    before `apply`, off the tape, and enter as non-differentiable vectors: the backward accounts for their dependence on z (and
    of scale on gamma) analytically, as ps_bn_bwd defines it.  Forward: ps_bn_apply, the inference call's bits.  Saved: z and the
    column vectors; neither t nor y.  Backward: one ps_bn_bwd -- gz only if z needs it, dgamma / dbeta only if gamma or beta does.
    No float atomics, nothing waits for the host: the same bits on every run."""

    @staticmethod
    def forward(ctx, z, gamma, beta, mean, var, scale, eps, relu, l2norm):
        ctx.eps, ctx.relu, ctx.l2norm = eps, relu, l2norm
        z = z.contiguous()
        ctx.save_for_backward(z, mean, var, scale, beta)
        return batch_norm_apply(z, mean, scale, beta, relu, l2norm)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        z, mean, var, scale, beta = ctx.saved_tensors
        need = ctx.needs_input_grad
        gy = gy.contiguous()                                          # y.sum().backward() hands over a stride-0 tensor
        gz, dgamma, dbeta = batch_norm_bwd(z, gy, mean, var, scale, beta, ctx.eps, ctx.relu, ctx.l2norm, need_gz=need[0],
                                           need_affine=need[1] or need[2])
        return gz, dgamma if need[1] else None, dbeta if need[2] else None, None, None, None, None, None, None


def _live_vec(live, m, device):
    if live is None:
        return None
    if live.dtype != torch.int32 or live.dim() != 1 or live.numel() != m or live.device != device:
        raise ValueError(f"live must be an int32 [{m}] vector on the device of x")
    return live.contiguous()


def layer_norm_fwd(x, gamma, beta, eps, live=None, out=None, stats=True):
    """(y [M, N], mean [M], rstd [M]) of F.layer_norm over the last dimension of x [M, N] (ps_layer_norm): one wave per row, two
    passes in fp32 (the mean, then the centred squares).  live: int32 [M] or None; a row with live <= 0 is not read and gives
    zeros (y, mean and rstd).  stats=False: mean and rstd are None and not written.  out: a contiguous fp32 [M, N] device tensor
    to write into; out=x works in place and gives the bits of a new tensor."""
    _require_cuda(x, gamma, beta, live, out)
    if x.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if x.dim() != 2:
        raise ValueError("2-D matrix expected")
    if out is None or out is not x:
        x = x.contiguous()
    elif not x.is_contiguous():
        raise ValueError("in place: x must be contiguous")
    M, N = x.size(0), x.size(1)
    gamma, beta = (_fp32_vec(n, t, N, x.device) for n, t in (("gamma", gamma), ("beta", beta)))
    live = _live_vec(live, M, x.device)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, N) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous fp32 [M, N] tensor on the device of x")
    mean = rstd = None
    if stats:
        mean, rstd = (torch.empty(M, dtype=torch.float32, device=x.device) for _ in range(2))
    with torch.cuda.device(x.device):
        nv.call("ps_layer_norm", nv.ptr(x), M, N, nv.ptr(gamma), nv.ptr(beta), float(eps), nv.ptr(live), nv.ptr(out), nv.ptr(mean),
                nv.ptr(rstd), nv.stream())
    return out, mean, rstd


def layer_norm_bwd(x, gy, mean, rstd, gamma, live=None, need_gx=True, need_affine=True, out=None):
    """(gx [M, N], dgamma [N], dbeta [N]) of layer_norm_fwd for the same x, mean, rstd, gamma and live (ps_layer_norm_bwd).  xh is
    recomputed from x with the forward's bits; the column sums are fp64 in a fixed order; the workspace comes from torch's
    allocator.  need_gx / need_affine False: that output is None and not computed.  out: a contiguous fp32 [M, N] device tensor
    for gx; out=gy works in place."""
    _require_cuda(x, gy, mean, rstd, gamma, live, out)
    if x.dtype != torch.float32 or gy.dtype != torch.float32:
        raise TypeError("fp32 expected")
    if x.dim() != 2 or x.shape != gy.shape:
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} vs gy {tuple(gy.shape)}")
    x = x.contiguous()
    M, N = x.size(0), x.size(1)
    gamma = _fp32_vec("gamma", gamma, N, x.device)
    mean, rstd = (_fp32_vec(n, t, M, x.device) for n, t in (("mean", mean), ("rstd", rstd)))
    live = _live_vec(live, M, x.device)
    gx = dgamma = dbeta = None
    if out is None:
        gy = gy.contiguous()
        if need_gx:
            gx = torch.empty((M, N), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, N) or not out.is_contiguous() or not gy.is_contiguous() \
            or out.device != x.device:
        raise ValueError("out must be a contiguous fp32 [M, N] tensor on the device of x (and gy contiguous)")
    elif need_gx:
        gx = out
    ws, wsb = None, 0
    if need_affine:
        dgamma, dbeta = (torch.empty(N, dtype=torch.float32, device=x.device) for _ in range(2))
        ws, wsb = nv.workspace("ps_layer_norm_bwd_workspace_bytes", x.device, M, N)
    with torch.cuda.device(x.device):
        nv.call("ps_layer_norm_bwd", nv.ptr(x), nv.ptr(gy), M, N, nv.ptr(mean), nv.ptr(rstd), nv.ptr(gamma), nv.ptr(live), nv.ptr(gx),
                nv.ptr(dgamma), nv.ptr(dbeta), nv.ptr(ws), wsb, nv.stream())
    return gx, dgamma, dbeta


def layer_norm_torch(x, gamma, beta, eps=1e-5, live=None):
    """layer_norm() as a differentiable torch expression (grad_method "torch", other dtypes, CPU tensors)"""
    y = F.layer_norm(x, (x.size(-1),), gamma, beta, eps)
    if live is None:
        return y
    return torch.where((live > 0).unsqueeze(-1), y, torch.zeros_like(y))


def layer_norm(x, gamma, beta, eps=1e-5, live=None):
    """F.layer_norm over the last dimension of x [M, N], zeros in the rows whose `live` (int32 [M], optional) is not positive.
    Off the tape: one ps_layer_norm into a new tensor, without statistics.  With autograd on and x, gamma or beta requiring a
    gradient the call stays on the tape: LayerNormFn (the same kernel forward, ps_layer_norm_bwd backward) for CUDA fp32 operands
    under sampling.grad_method == "hip", layer_norm_torch elsewhere ("torch", other dtypes, CPU tensors; a backward that is itself
    to be differentiated needs "torch" too: LayerNormFn is once-differentiable)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, gamma, beta)):
        from .graph import use_hip_grad
        if x.dim() == 2 and use_hip_grad(x, gamma, beta) and (live is None or live.is_cuda):
            return LayerNormFn.apply(x, gamma, beta, float(eps), live)
        return layer_norm_torch(x, gamma, beta, eps, live)
    return layer_norm_fwd(x, gamma, beta, eps, live, stats=False)[0]


class LayerNormFn(torch.autograd.Function):
    """Differentiable layer_norm() for CUDA fp32 operands.  Forward: ps_layer_norm with its statistics -- the inference call's
    bits.  Saved: x, mean, rstd, gamma and live; neither xh nor y.  Backward: one ps_layer_norm_bwd -- gx only if x needs it,
    dgamma / dbeta only if gamma or beta does.  No float atomics, nothing waits for the host: the same bits on every run."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, live):
        x = x.contiguous()
        y, mean, rstd = layer_norm_fwd(x, gamma, beta, eps, live)
        ctx.save_for_backward(x, mean, rstd, gamma, live)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, mean, rstd, gamma, live = ctx.saved_tensors
        need = ctx.needs_input_grad
        gy = gy.contiguous()                                          # y.sum().backward() hands over a stride-0 tensor
        gx, dgamma, dbeta = layer_norm_bwd(x, gy, mean, rstd, gamma, live, need_gx=need[0], need_affine=need[1] or need[2])
        return gx, dgamma if need[1] else None, dbeta if need[2] else None, None, None


GCN_MIN_ROWS, GCN_MAX_T = 64 * 384, 16     # the M / T gates of ps_gcn_layer: gcn_orders makes no order the layer call would refuse


def gcn_orders(ids, nvalid, max_idx):
    """The row orders of ps_gcn_layer for several layers in ONE launch (ps_gcn_order): ids / nvalid are lists of the layers'
    [M, T] / [M] int32 tensors, max_idx the bound the layer calls will pass (at most h_full.size(0) - 1).  Returns one
    (ord, tile_heavy) pair per layer for gcn_layer(order=...), or None where ps_gcn_layer does not serve the shape.  The slices
    walk_sample_layers returns are passed as the one buffer they are; anything else is stacked first."""
    _require_cuda(*ids, *nvalid)
    layers, M, T = len(ids), ids[0].size(0), ids[0].size(1)
    if layers == 0 or M < GCN_MIN_ROWS or T > GCN_MAX_T:
        return None
    if any(t.shape != (M, T) or t.dtype != torch.int32 for t in ids) or any(t.shape != (M,) or t.dtype != torch.int32 for t in nvalid):
        raise ValueError("shape mismatch")

    def one_buffer(ts):
        step = ts[0].numel() * 4
        if all(t.is_contiguous() and t.data_ptr() == ts[0].data_ptr() + r * step for r, t in enumerate(ts)):
            return ts[0]                                 # consecutive slices: the first one's pointer is the buffer's
        return torch.stack(ts)
    ids_all, nv_all = one_buffer(ids), one_buffer(nvalid)
    dev = ids[0].device
    ntiles = (M + 63) // 64
    ord_ = torch.empty((layers, ntiles * 64), dtype=torch.int32, device=dev)
    heavy = torch.empty((layers, ntiles), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nv.call("ps_gcn_order", nv.ptr(ids_all), nv.ptr(nv_all), layers, M, T, int(max_idx), nv.ptr(ord_), nv.ptr(heavy), nv.stream())
    return [(ord_[r], heavy[r]) for r in range(layers)]


def gcn_layer(x, W, b, h_full, ids, counts, nvalid, W2, wts=None, max_idx=None, renorm=True, relu=True, l2norm=True, order=None):
    """linear(x, W, b, x2=importance_pool(h_full, ids, counts, wts, nvalid, max_idx, renorm), W2=W2, relu, l2norm) -- the same
    bits -- in two launches (row order, GEMM) where ps_gcn_layer serves the shape (rows that keep no neighbour skip the W2 half,
    the pooled rows are not written out); elsewhere, and under PS_GCN_FUSED=0, as that pair of calls.  W / W2: matrices or
    StagedWeights (both or neither).  order: this layer's (ord, tile_heavy) of gcn_orders, made from the same ids / nvalid /
    max_idx -- the call is then the GEMM launch alone (ps_gcn_layer_ordered)."""
    from . import sampling
    staged = isinstance(W, StagedWeight)
    if isinstance(W2, StagedWeight) != staged:
        raise ValueError("W and W2 must both be staged or both plain")
    Wm, W2m = (W.t, W2.t) if staged else (W, W2)
    _require_cuda(x, Wm, b, h_full, W2m, ids, counts, wts, nvalid)
    x, h_full = x.contiguous(), h_full.contiguous()
    if x.dtype != torch.float32 or h_full.dtype != torch.float32:
        raise TypeError("fp32 expected")
    M, K, n_full, H = x.size(0), x.size(1), h_full.size(0), h_full.size(1)
    Wk, ldw = _rowmajor(Wm)
    W2k, ldw2 = _rowmajor(W2m)
    N = Wk.size(0)
    if Wk.size(1) != K or W2k.size(1) != H or W2k.size(0) != N or ids.size(0) != M:
        raise ValueError("shape mismatch")
    T = ids.size(1)
    if max_idx is None:
        max_idx = n_full - 1
    if b is not None:
        b = b.contiguous()
    ids, nvalid = ids.contiguous(), nvalid.contiguous()
    counts = counts.contiguous() if counts is not None else None
    wts = wts.contiguous() if wts is not None else None
    flags = (nv.PS_RELU if relu else 0) | (nv.PS_L2NORM if l2norm else 0) | (nv.PS_WPERM if staged else 0)
    ws, wsb = nv.workspace("ps_gcn_layer_workspace_bytes", x.device, M, H)
    if wsb > 0:
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        if order is not None:
            ord_, heavy = order
            if ord_.dtype != torch.int32 or heavy.dtype != torch.int32 or ord_.numel() != (M + 63) // 64 * 64 \
                    or heavy.numel() != (M + 63) // 64:
                raise ValueError("order: (int32[64 * ceil(M / 64)], int32[ceil(M / 64)]) of gcn_orders expected")
        with torch.cuda.device(x.device):
            if order is not None:
                rc = nv.lib().ps_gcn_layer_ordered(nv.ptr(x), M, K, nv.ptr(Wk, contiguous=False), ldw, nv.ptr(b), N, nv.ptr(h_full),
                                                   n_full, H, nv.ptr(ids), nv.ptr(counts), nv.ptr(wts), nv.ptr(nvalid), T, int(max_idx),
                                                   int(renorm), nv.ptr(W2k, contiguous=False), ldw2, flags, nv.ptr(y), nv.ptr(ws), wsb,
                                                   nv.ptr(ord_), nv.ptr(heavy), nv.stream())
            else:
                rc = nv.lib().ps_gcn_layer(nv.ptr(x), M, K, nv.ptr(Wk, contiguous=False), ldw, nv.ptr(b), N, nv.ptr(h_full), n_full, H,
                                           nv.ptr(ids), nv.ptr(counts), nv.ptr(wts), nv.ptr(nvalid), T, int(max_idx), int(renorm),
                                           nv.ptr(W2k, contiguous=False), ldw2, flags, nv.ptr(y), nv.ptr(ws), wsb, nv.stream())
        if rc != nv.PS_EUNSUPPORTED:
            nv.check(rc, "ps_gcn_layer")
            return y
    h_neigh = sampling.importance_pool(h_full, ids=ids, counts=counts, wts=wts, nvalid=nvalid, max_idx=max_idx, renorm=renorm)
    return linear(x, W, b, x2=h_neigh, W2=W2, relu=relu, l2norm=l2norm)


def lsh_encode(x, A, planes=False):
    """codes uint8[n, nbits/8]: bit j = (x . A[j] >= 0), LSB first (faiss IndexLSH.sa_encode).  A: matrix, StagedWeight or
    StagedLsh.  planes=True: -> (codes, lsh_expand(codes)), from the encode launch itself where ps_lsh_encode_planes serves
    the call (a StagedLsh, whole 64-bit code words), else as the two launches."""
    flags = nv.PS_LSH_STAGED if isinstance(A, StagedLsh) else nv.PS_WPERM if isinstance(A, StagedWeight) else 0
    if flags == nv.PS_LSH_STAGED:
        nbits, da, A = A.shape[0], A.shape[1], A.image
    elif flags:
        A = A.t
    _require_cuda(x, A)
    x = x.contiguous()
    A = A.contiguous()
    n, d = x.size(0), x.size(1)
    if flags != nv.PS_LSH_STAGED:
        nbits, da = A.size(0), A.size(1)
    if da != d:
        raise ValueError("projection matrix must be [nbits, dim]")
    codes = torch.empty((n, nbits // 8), dtype=torch.uint8, device=x.device)
    if planes and flags == nv.PS_LSH_STAGED:
        pl, nb = nv.workspace("ps_lsh_planes_bytes", x.device, n, nbits // 8)
        if nb:
            with torch.cuda.device(x.device):
                rc = nv.call("ps_lsh_encode_planes", nv.ptr(x), n, d, nv.ptr(A), nbits, nv.ptr(codes), nv.ptr(pl), nv.stream(),
                             unsupported_ok=True)
            if rc == nv.PS_OK:
                return codes, pl
    with torch.cuda.device(x.device):
        nv.call("ps_lsh_encode", nv.ptr(x), n, d, nv.ptr(A), nbits, nv.ptr(codes), flags, nv.stream())
    return (codes, lsh_expand(codes)) if planes else codes


HAMMING_MAX_K = 64        # ps_hamming_topk (popcount scan); the MFMA scan serves k <= 32; beyond 64: _hamming_topk_large_k


def lsh_expand(codes):
    """Sign planes of a code table (uint8 [n, cs] -> +1/-1 bytes in MFMA fragment order, see csrc/hamming_mfma.hip);
    None when the code size is not a multiple of 4 bytes."""
    _require_cuda(codes)
    codes = codes.contiguous()
    n, cs = codes.size(0), codes.size(1)
    planes, nb = nv.workspace("ps_lsh_planes_bytes", codes.device, n, cs)
    if nb:
        with torch.cuda.device(codes.device):
            nv.call("ps_lsh_expand", nv.ptr(codes), n, cs, nv.ptr(planes), nv.stream())
    return planes


def hamming_mfma_supported(nq, N, cs, k):
    return nv.lib().ps_hamming_topk_mfma_workspace_bytes(nq, N, cs, k) > 0


def hamming_topk(qcodes, codes, k, id_offset=0, planes=None, use_mfma=True, out=None):
    """-> (dist int32[nq,k], ids int64[nq,k]): k smallest by (distance, id), ascending.
    out=(dist, ids): write into these contiguous device tensors (a rank's candidate record, shard.py) instead of new ones.
    `planes` = lsh_expand(codes), kept by the index: the scan then runs as an exact int8 MFMA contraction when the
    shape is served (ps_hamming_topk_mfma); otherwise, and for `use_mfma=False`, the popcount kernel runs.  Both
    return the same bits."""
    _require_cuda(qcodes, codes)
    qcodes = qcodes.contiguous()
    codes = codes.contiguous()
    nq, cs = qcodes.size(0), qcodes.size(1)
    N = codes.size(0)
    if out is not None:
        dist, ids = out
        if (tuple(dist.shape) != (nq, k) or tuple(ids.shape) != (nq, k) or dist.dtype != torch.int32
                or ids.dtype != torch.int64 or not dist.is_contiguous() or not ids.is_contiguous()):
            raise ValueError("out must be contiguous (int32 [nq, k], int64 [nq, k])")
    if k > HAMMING_MAX_K or cs > 128 or (cs & (cs - 1)) != 0 or cs % 4 != 0:
        # beyond the scans' shapes (k > 64; codes longer than 1024 bits or not 32 * 2^j bits): exact L2 over the +-1 images
        d, i = _hamming_topk_large_k(qcodes, codes, k, id_offset)
        if out is None:
            return d, i
        dist.copy_(d)
        ids.copy_(i)
        return dist, ids
    if out is None:
        dist = torch.empty((nq, k), dtype=torch.int32, device=qcodes.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=qcodes.device)
    if use_mfma and planes is not None:
        ws, wsb = nv.workspace("ps_hamming_topk_mfma_workspace_bytes", qcodes.device, nq, N, cs, k)
        if wsb > 0:
            with torch.cuda.device(qcodes.device):
                # the queries go in as packed codes: the scan's workgroups build their own sign planes
                nv.call("ps_hamming_topk_mfma_codes", nv.ptr(qcodes), nq, nv.ptr(planes), N, cs, k, id_offset, nv.ptr(dist),
                        nv.ptr(ids), nv.ptr(ws), wsb, nv.stream())
            return dist, ids
    ws, wsb = nv.workspace("ps_hamming_topk_workspace_bytes", qcodes.device, nq, N, cs, k)
    with torch.cuda.device(qcodes.device):
        nv.call("ps_hamming_topk", nv.ptr(qcodes), nq, nv.ptr(codes if N else None), N, cs, k, id_offset, nv.ptr(dist),
                nv.ptr(ids), nv.ptr(ws), wsb, nv.stream())
    return dist, ids


LARGE_K_SIGN_BYTES = 8 << 30      # budget for the +-1 float image of the code table in the k > 64 path


def _signs(codes):
    """uint8 [n, cs] -> float32 [n, 8 cs] of +-1 (any fixed bit order: both operands use the same)"""
    shifts = torch.arange(8, device=codes.device, dtype=torch.uint8)
    bits = (codes.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(codes.size(0), -1).to(torch.float32) * 2.0 - 1.0


def _hamming_topk_large_k(qcodes, codes, k, id_offset):
    """k > 64 (faiss.IndexLSH.search accepts any k): between +-1 vectors the squared L2 distance is 4 x the Hamming distance
    -- small integers, exact in fp32 -- so the exact L2 search (ps_l2_topk: fp32-MFMA GEMM + multi-sweep row top-k, any k,
    ties by id) returns the same (distance, id) order as the scans.  Costs a float image of the table (2 KiB per 512-bit
    code): meant for the occasional large request, not for the hot path."""
    N, nbits = codes.size(0), codes.size(1) * 8
    if N * nbits * 4 > LARGE_K_SIGN_BYTES:
        raise ValueError(f"LSH search with k = {k} > {HAMMING_MAX_K} expands the code table to floats "
                         f"({N * nbits * 4 / 2 ** 30:.1f} GiB here, limit {LARGE_K_SIGN_BYTES >> 30} GiB): split the table or the request")
    d2, ids = l2_topk(_signs(codes), _signs(qcodes), k)
    missing = ids < 0
    dist = torch.where(missing, torch.full_like(d2, 0.0), d2 * 0.25).round().to(torch.int32)
    dist[missing] = 0x7fffffff
    ids = torch.where(missing, ids, ids + int(id_offset))
    return dist, ids


def topk_merge(dist_in, ids_in):
    """[P, nq, k] candidate lists -> global [nq, k] by (distance, id)."""
    dist_in = dist_in.contiguous()
    ids_in = ids_in.contiguous()
    P, nq, k = dist_in.shape
    dist = torch.empty((nq, k), dtype=torch.int32, device=dist_in.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=dist_in.device)
    with torch.cuda.device(dist_in.device):
        nv.call("ps_topk_merge", nv.ptr(dist_in), nv.ptr(ids_in), P, nq, k, nv.ptr(dist), nv.ptr(ids), nv.stream())
    return dist, ids


def topk_merge_records(records, nq, k):
    """records uint8 [P, rec]: shard p's candidate record = [nq*k int64 ids | nq*k int32 distances | pad to 16 B], exactly
    as one all-gather delivers them -> global (dist int32[nq,k], ids int64[nq,k]) by (distance, id); no repacking."""
    if records.dtype != torch.uint8 or records.dim() != 2 or not records.is_contiguous():
        raise ValueError("records must be a contiguous uint8 [P, record_bytes] tensor")
    P, rec = records.shape
    nq, k = int(nq), int(k)
    n = nq * k
    if rec < 12 * n or rec % 8 != 0:
        raise ValueError("record too short or not 8-byte aligned")
    dist = torch.empty((nq, k), dtype=torch.int32, device=records.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=records.device)
    base = records.data_ptr()
    with torch.cuda.device(records.device):
        nv.call("ps_topk_merge_strided", base + 8 * n, rec // 4, base, rec // 8, P, nq, k, nv.ptr(dist), nv.ptr(ids), nv.stream())
    return dist, ids


def dot_topk(E, qidx, k, exclude_self=True):
    """Exact search: top-k of E[q] @ E.T per query row index (reference inference.py:112-118)."""
    E = E.contiguous()
    qidx = qidx.to(device=E.device, dtype=torch.int64).contiguous()
    N, D = E.size(0), E.size(1)
    nq = qidx.numel()
    if k < 1:
        raise ValueError(f"k must be positive, got {k}")
    vals = torch.empty((nq, k), dtype=torch.float32, device=E.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=E.device)
    ws, wsb = nv.workspace("ps_dot_topk_workspace_bytes", E.device, nq, N, D, k)
    with torch.cuda.device(E.device):
        nv.call("ps_dot_topk", nv.ptr(E), N, D, nv.ptr(qidx), nq, k, int(exclude_self), nv.ptr(vals), nv.ptr(ids), nv.ptr(ws), wsb,
                nv.stream())
    return vals, ids


def _fp32_rows(E):
    _require_cuda(E)
    if E.dtype != torch.float32 or E.dim() != 2:
        raise TypeError("fp32 [N, D] matrix expected")
    return E.contiguous()


def row_dot(A, ia, B, ib):
    """out[i] = A[ia[i]] . B[ib[i]] (ps_row_dot): the arithmetic of linear() / dot_topk(), so out[i] is bit-identical to the
    entry linear(A[ia], B)[i, ib[i]].  An index outside the matrix gives NaN."""
    A, B = _fp32_rows(A), _fp32_rows(B)
    if A.size(1) != B.size(1):
        raise ValueError(f"shape mismatch: A {tuple(A.shape)} vs B {tuple(B.shape)}")
    ia = ia.to(device=A.device, dtype=torch.int64).contiguous()
    ib = ib.to(device=A.device, dtype=torch.int64).contiguous()
    if ia.numel() != ib.numel():
        raise ValueError("ia and ib must have the same length")
    out = torch.empty(ia.numel(), dtype=torch.float32, device=A.device)
    with torch.cuda.device(A.device):
        nv.call("ps_row_dot", nv.ptr(A), A.size(0), nv.ptr(B), B.size(0), A.size(1), nv.ptr(ia), nv.ptr(ib), ia.numel(), nv.ptr(out),
                nv.stream())
    return out


def rerank_max_candidates():
    """the longest candidate list rerank_topk takes (ps_rerank_max_candidates: the library's own figure)"""
    return int(nv.lib().ps_rerank_max_candidates())


def rerank_topk(E, Q, cand, k, id_offset=0):
    """The second level of a two-level search (ps_rerank_topk): cand int64 [nq, R] holds every query's candidate ids as a
    first-level search returned them (hamming_topk; -1 pads and ids outside id_offset .. id_offset + N - 1 are skipped, an id
    listed twice counts once) -> (vals fp32 [nq, k], ids int64 [nq, k]): the k best candidates by the exact inner product
    Q[i] . E[id - id_offset], in dot_topk's order (descending, ties by ascending id) and with its bits, padded with (-inf, -1)."""
    E, Q = _fp32_rows(E), _fp32_rows(Q)
    if E.size(1) != Q.size(1):
        raise ValueError(f"shape mismatch: E {tuple(E.shape)} vs Q {tuple(Q.shape)}")
    if cand.dim() != 2 or cand.size(0) != Q.size(0):
        raise ValueError(f"cand must be [nq, R] with one row per query, got {tuple(cand.shape)} for {Q.size(0)} queries")
    if k < 1:
        raise ValueError(f"k must be positive, got {k}")
    cand = cand.to(device=E.device, dtype=torch.int64).contiguous()
    nq, R = cand.size(0), cand.size(1)
    if not 1 <= R <= rerank_max_candidates():
        raise ValueError(f"rerank_topk takes 1 .. {rerank_max_candidates()} candidates per query, got {R}")
    vals = torch.empty((nq, k), dtype=torch.float32, device=E.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=E.device)
    with torch.cuda.device(E.device):
        nv.call("ps_rerank_topk", nv.ptr(E), E.size(0), E.size(1), int(id_offset), nv.ptr(Q), nq, nv.ptr(cand), R, int(k),
                nv.ptr(vals), nv.ptr(ids), nv.stream())
    return vals, ids


def rank_count(E, Q, thr, tid, id_offset=0, count=None):
    """count[i] += #{items j of E (ids id_offset + j) that precede (thr[i], tid[i]) in dot_topk's order of Q[i] . E^T}
    (ps_rank_count: similarity descending by float key, ties by ascending id).  One GEMM with a counting epilogue, no [nq, N]
    slab.  count: int64 [nq] on the device (a new zero vector when None); calls over disjoint item ranges add up."""
    E, Q = _fp32_rows(E), _fp32_rows(Q)
    if E.size(1) != Q.size(1):
        raise ValueError(f"shape mismatch: E {tuple(E.shape)} vs Q {tuple(Q.shape)}")
    nq = Q.size(0)
    thr = thr.to(device=Q.device, dtype=torch.float32).contiguous()
    tid = tid.to(device=Q.device, dtype=torch.int64).contiguous()
    if thr.numel() != nq or tid.numel() != nq:
        raise ValueError("thr and tid need one entry per query row")
    if count is None:
        count = torch.zeros(nq, dtype=torch.int64, device=Q.device)
    elif count.dtype != torch.int64 or not count.is_contiguous() or count.numel() != nq or count.device != Q.device:
        raise ValueError("count must be a contiguous int64 [nq] tensor on the queries' device")
    with torch.cuda.device(Q.device):
        nv.call("ps_rank_count", nv.ptr(E), E.size(0), E.size(1), int(id_offset), nv.ptr(Q), nq, nv.ptr(thr), nv.ptr(tid),
                nv.ptr(count), nv.stream())
    return count


def target_rank(E, qidx, gt, id_offset=0):
    """1-based rank of item gt[i] in the similarity order of query row qidx[i] over all rows of E (dot_topk's order:
    similarity descending, ties by ascending id), int64 on the device.  qidx / gt are row indices of E in [0, N); E's row j
    has the id id_offset + j (ties compare those ids, so the ranks do not depend on it -- the offset matters to rank_count
    over item ranges).  rank <= k  <=>  gt[i] is in dot_topk(E, qidx, k, exclude_self=False)[1][i]."""
    E = _fp32_rows(E)
    qidx = qidx.to(device=E.device, dtype=torch.int64).contiguous()
    gt = gt.to(device=E.device, dtype=torch.int64).contiguous()
    if qidx.numel() != gt.numel():
        raise ValueError("qidx and gt must have the same length")
    N = E.size(0)
    for name, t in (("qidx", qidx), ("gt", gt)):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= N):
            raise IndexError(f"{name} holds a row index outside [0, {N})")
    Q = E.index_select(0, qidx)
    thr = row_dot(E, qidx, E, gt)
    count = rank_count(E, Q, thr, gt + int(id_offset), id_offset)
    return count + 1


def l2_topk(X, Q, k, assign=None, probe=None):
    """k nearest by squared L2 (IndexFlatL2 / IndexIVFFlat scan): -> (dist fp32[nq,k], ids int64[nq,k])."""
    X = X.contiguous()
    Q = Q.to(X.device).contiguous()
    N, D = X.size(0), X.size(1)
    nq = Q.size(0)
    if k < 1:
        raise ValueError(f"k must be positive, got {k}")
    dist = torch.empty((nq, k), dtype=torch.float32, device=X.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=X.device)
    ws, wsb = nv.workspace("ps_l2_topk_workspace_bytes", X.device, nq, N, D, k)
    words = probe.size(1) if probe is not None else 0
    with torch.cuda.device(X.device):
        nv.call("ps_l2_topk", nv.ptr(X), N, D, nv.ptr(Q), nq, k, nv.ptr(assign), nv.ptr(probe), words, nv.ptr(dist), nv.ptr(ids),
                nv.ptr(ws), wsb, nv.stream())
    return dist, ids


def ivf_topk(Xs, list_ptr, item_ids, Q, probes, k, max_list=None):
    """Inverted-file scan (ps_ivf_topk): Xs fp32 [N, D] sorted by list, list_ptr int64 [nlist + 1], item_ids int64 [N] (original
    id of every sorted row), probes int32 [nq, nprobe] -> (dist fp32 [nq, k], ids int64 [nq, k]) by (squared L2, original id).
    max_list = the longest list (computed here with one host sync when not given: an index knows it from `add`)."""
    Xs = Xs.contiguous()
    Q = Q.to(Xs.device).contiguous()
    probes = probes.to(device=Xs.device, dtype=torch.int32).contiguous()
    list_ptr = list_ptr.to(device=Xs.device, dtype=torch.int64).contiguous()
    item_ids = item_ids.to(device=Xs.device, dtype=torch.int64).contiguous()
    N, D = Xs.size(0), Xs.size(1)
    nq, nprobe, nlist = Q.size(0), probes.size(1), list_ptr.numel() - 1
    if k < 1:
        raise ValueError(f"k must be positive, got {k}")
    if probes.size(0) != nq or item_ids.numel() != N or Q.size(1) != D:
        raise ValueError("shape mismatch")
    if max_list is None:
        max_list = (list_ptr[1:] - list_ptr[:-1]).max().item() if nlist else 0
    max_list, k = int(max_list), int(k)
    dist = torch.empty((nq, k), dtype=torch.float32, device=Xs.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=Xs.device)
    ws, wsb = nv.workspace("ps_ivf_topk_workspace_bytes", Xs.device, nq, N, D, k, nlist, nprobe, max_list)
    with torch.cuda.device(Xs.device):
        nv.call("ps_ivf_topk", nv.ptr(Xs), N, D, nv.ptr(list_ptr), nlist, max_list, nv.ptr(item_ids), nv.ptr(Q), nq, nv.ptr(probes),
                nprobe, k, nv.ptr(dist), nv.ptr(ids), nv.ptr(ws), wsb, nv.stream())
    return dist, ids


_jump_polys_dev = {}


def _jump_polys(dev):
    key = str(dev)
    if key not in _jump_polys_dev:
        from . import mtjump
        import numpy as np
        _jump_polys_dev[key] = torch.from_numpy(mtjump.jump_polynomials().view(np.int32)).to(dev).contiguous()
    return _jump_polys_dev[key]


_radix_polys_dev = {}


def _radix_polys(dev):
    key = str(dev)
    if key not in _radix_polys_dev:
        from . import mtjump
        import numpy as np
        cl2 = nv.lib().ps_mt19937_chunk_log2()
        _radix_polys_dev[key] = torch.from_numpy(mtjump.radix_polynomials(cl2).view(np.int32)).to(dev).contiguous()
    return _radix_polys_dev[key]


_window_polys_dev = {}


def _window_polys(dev):
    key = str(dev)
    if key not in _window_polys_dev:
        from . import mtjump
        import numpy as np
        cl2, shift = nv.lib().ps_mt19937_chunk_log2(), nv.lib().ps_mt19937_window_shift()
        _window_polys_dev[key] = torch.from_numpy(mtjump.window_polynomials(cl2, shift=shift).view(np.int32)).to(dev).contiguous()
    return _window_polys_dev[key]


_pending_state = []
_handback_host = {}          # device -> pinned int32[625]: the state's 624 words, then pos (one hand-back in flight at most)


def _handback_buffer(dev):
    key = str(dev)
    if key not in _handback_host:
        _handback_host[key] = torch.empty(625, dtype=torch.int32).pin_memory()
    return _handback_host[key]


def finish_rng_state():
    """Completes a deferred hand-back of the np.random state (mt19937_random_sample(advance='defer')): waits for the
    624-word state copy (an event, not a device synchronisation) and installs it with np.random.set_state.  Called by
    the code that asked for the deferral before it returns to the caller, so user code always sees the advanced state."""
    import numpy as np
    while _pending_state:
        name, has_gauss, cached, host, ev = _pending_state.pop()
        ev.synchronize()
        words = host.numpy().view(np.uint32).copy()              # the pinned buffer is reused by the next hand-back
        np.random.set_state((name, words[:624], int(words[624]), has_gauss, cached))


def mt19937_random_sample(n, device, skip=0, advance=True, parallel=True, radix=True, raw=False, one_round=True, ranges=None):
    """n doubles of the process-global numpy legacy stream generated ON THE DEVICE (after skipping `skip`
    doubles); with advance=True the global np.random state is advanced exactly as
    `np.random.random_sample(skip + n)` would (reference utils/random_walk.py:79 draws these one at a time).
    advance='defer': the state comes back through an asynchronous copy that `finish_rng_state()` completes -- the host
    keeps enqueueing the kernels that consume the uniforms instead of waiting for the generator (the caller must call
    finish_rng_state() before returning to code that may touch np.random).
    raw=True (skip = 0, n >= 2^17): returns the stream as untempered MT19937 words, int32[2n + 1248], for the walk kernels'
    PS_RNG_STREAM_RAW mode (uniform i = words 2i, 2i + 1) instead of doubles.
    ranges (raw only): up to three runs (lo, hi) of uniform indices the caller will read; only those words of the buffer are
    generated (item shards: the stream positions of a rank's own start nodes), the np.random state still advances by n."""
    import numpy as np
    name, key, pos, has_gauss, cached = np.random.get_state()
    if name != "MT19937":
        raise RuntimeError("numpy global RNG is not MT19937")
    dev = torch.device(device)
    # pinned staging + asynchronous copy: a pageable `.to(dev)` waits for the stream, i.e. for the whole previous step
    if os.environ.get("PS_MT_SYNC_UPLOAD") == "1":
        st_in = torch.from_numpy(key.astype(np.uint32).view(np.int32)).to(dev)
    else:
        st_in = torch.from_numpy(key.astype(np.uint32).view(np.int32)).pin_memory().to(dev, non_blocking=True)
    st_out = torch.empty(625, dtype=torch.int32, device=dev)          # 624 state words, then pos: one buffer, one copy back
    pos_out = st_out[624:]
    if raw and (skip != 0 or not parallel or n < (1 << 17)):
        raise ValueError("raw stream: skip = 0, the parallel generator and n >= 2^17 are required")
    n, skip, pos = int(n), int(skip), int(pos)
    out = torch.empty(2 * n + 1248, dtype=torch.int32, device=dev) if raw else torch.empty(n, dtype=torch.float64, device=dev)
    polys = _jump_polys(dev) if parallel else None
    rpolys = _radix_polys(dev) if (parallel and radix) else None      # radix=False: windows by doubling
    wpolys = _window_polys(dev) if (parallel and radix and one_round) else None    # one_round=False: two radix-32 rounds
    ws, wsb = nv.workspace("ps_mt19937_workspace_bytes", dev, skip, n) if parallel else (None, 0)
    if ranges is not None and not raw:
        raise ValueError("ranges: raw stream only")
    rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2)) if ranges is not None and len(ranges) else None
    if rg is not None and rg.shape[0] > 3:
        rg = None                                                    # more runs than the planner takes: generate everything
    if rg is not None and os.environ.get("PS_MT_POISON") == "1":
        # debug aid (tests): words outside the requested runs stay unwritten, and the caching allocator readily hands back a
        # block that still holds a same-seed stream from an earlier call -- a kernel that read outside its runs would then see
        # correct-looking words.  Poisoned, any such read changes the sampled ids deterministically.
        out.fill_(-1)
    levels, rlevels, nwin = (0 if t is None else t.size(0) for t in (polys, rpolys, wpolys))
    with torch.cuda.device(dev):
        if raw:
            nv.call("ps_mt19937_raw_stream", nv.ptr(st_in), pos, n, nv.ptr(out), nv.ptr(st_out), nv.ptr(pos_out), nv.ptr(polys),
                    levels, nv.ptr(rpolys), rlevels, nv.ptr(wpolys), nwin, rg.ctypes.data if rg is not None else None,
                    rg.shape[0] if rg is not None else 0, nv.ptr(ws), wsb, nv.stream())
        else:
            nv.call("ps_mt19937_random_sample", nv.ptr(st_in), pos, skip, n, nv.ptr(out), nv.ptr(st_out), nv.ptr(pos_out),
                    nv.ptr(polys), levels, nv.ptr(rpolys), rlevels, nv.ptr(wpolys), nwin, nv.ptr(ws), wsb, nv.stream())
    if advance == "defer":
        finish_rng_state()                                           # at most one hand-back in flight
        host = _handback_buffer(dev)
        with torch.cuda.device(dev):
            host.copy_(st_out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        _pending_state.append((name, has_gauss, cached, host, ev))
    elif advance:
        words = st_out.cpu().numpy().view(np.uint32)
        np.random.set_state((name, words[:624], int(words[624]), has_gauss, cached))
    return out
