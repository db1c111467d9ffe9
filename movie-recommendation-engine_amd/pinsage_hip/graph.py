"""DeviceGraph: the sampler's adjacency as CSR + per-row fp64 CDF resident in HBM.

Replaces RandomWalkSampler._prepare_adjacency_list (reference utils/random_walk.py:33-50) and
the per-step `weights / weights.sum()` + `np.random.choice` CDF (:72-79)."""
from __future__ import annotations

import os

import torch

from . import native as nv


class DeviceGraph:
    DEST_INFO_MIN_NODES = 8 << 20        # 64 MiB of node records: beyond what the L2s and most of the MALL hold next to the row data

    def __init__(self, edge_index, edge_weights=None, device=None, buckets=None, dest_info=None):
        dev = nv.require_gpu() if device is None else torch.device(device)
        ei = torch.as_tensor(edge_index)
        if ei.dim() != 2 or ei.size(0) != 2:
            raise ValueError("edge_index must have shape [2, num_edges]")
        E = int(ei.size(1))
        ei = ei.to(device=dev, dtype=torch.int64)
        src = ei[0].contiguous()
        dst = ei[1].contiguous()
        if E:
            mx = int(ei.max().item())          # reference: max_node_idx = edge_index.max().item() + 1
            if int(ei.min().item()) < 0:
                raise ValueError("negative node index in edge_index")
        else:
            mx = -1
        V = mx + 1
        if V >= 2 ** 31 or E >= 2 ** 32:
            raise ValueError("graph too large for int32 node ids / uint32 edge ids")
        w = None
        if edge_weights is not None:
            w = torch.as_tensor(edge_weights).to(device=dev, dtype=torch.float32).contiguous()
            if w.numel() != E:
                raise ValueError("edge_weights must have one entry per edge")
        self.device = dev
        self.V, self.E = V, E
        self.rowptr = torch.empty(V + 1, dtype=torch.int64, device=dev)
        self.col = torch.empty(E, dtype=torch.int32, device=dev)
        self.cdf = torch.empty(E, dtype=torch.float64, device=dev)
        wsorted = torch.empty(E, dtype=torch.float64, device=dev)
        ws, ws_bytes = nv.workspace("ps_csr_build_workspace_bytes", dev, E, V)
        with torch.cuda.device(dev):
            nv.call("ps_csr_build", nv.ptr(src), nv.ptr(dst), nv.ptr(w), E, V, nv.ptr(self.rowptr), nv.ptr(self.col),
                    nv.ptr(wsorted), nv.ptr(ws), ws_bytes, nv.stream())
            nv.call("ps_cdf_build", nv.ptr(self.rowptr), nv.ptr(wsorted), V, nv.ptr(self.cdf), nv.stream())
            # exact lookup accelerators for the walk kernels: packed (row start, degree) + bucket table
            self.nodeinfo = torch.empty(2 * V, dtype=torch.int32, device=dev)
            self.guide = torch.empty(E, dtype=torch.int32, device=dev)
            if E:
                nv.call("ps_guide_build", nv.ptr(self.rowptr), nv.ptr(self.cdf), V, nv.ptr(self.nodeinfo), nv.ptr(self.guide), nv.stream())
            self.packed = torch.empty(((E + 7) // 8) * 128, dtype=torch.uint8, device=dev)
            if E:
                nv.call("ps_pack_edges", nv.ptr(self.col), nv.ptr(self.cdf), nv.ptr(self.guide), E, nv.ptr(self.packed), nv.stream())
            # bucket records (one sector per later walk step).  Default: the 32-byte half records (four candidates' CDF entries as fp32
            # lower bounds + destinations) -- measured 5 % FASTER than the 64-byte records on SYN-25M too (0.406 against 0.431 ms per
            # two-layer launch, same box, alternating runs) at half the memory (1.6 GB instead of 3.2), and the only form that fits
            # BASELINE config 5 (64 GB beside the 66 GB graph); skipped when even they would not fit.  buckets = "full" / True builds
            # the 64-byte records (five exact candidates; kept as the cross-check), "half", False force a form.  The CSR build's
            # sort workspace is returned first: at 2 x 10^9 edges it is the size of the half records.
            del ws
            self.buckets, self.bucket_bytes = None, 0
            if E and buckets is not False:
                torch.cuda.empty_cache()
                free = torch.cuda.mem_get_info(dev)[0]
                form = {True: "full", "full": "full", "half": "half", None: None}[buckets]
                if form is None and os.environ.get("PS_GRAPH_BUCKETS") in ("full", "half"):     # experiments: force a form
                    form = os.environ["PS_GRAPH_BUCKETS"]
                if form is None:
                    form = "half" if E * 32 < (free * 3) // 5 else None
                if form == "full":
                    self.buckets, self.bucket_bytes = torch.empty(E * 64, dtype=torch.uint8, device=dev), 64
                    nv.call("ps_bucket_build", nv.ptr(self.rowptr), nv.ptr(self.col), nv.ptr(self.cdf), nv.ptr(self.guide), V, E,
                            nv.ptr(self.buckets), nv.stream())
                elif form == "half":
                    self.buckets, self.bucket_bytes = torch.empty(E * 32, dtype=torch.uint8, device=dev), 32
                    nv.call("ps_bucket_build_half", nv.ptr(self.rowptr), nv.ptr(self.col), nv.ptr(self.cdf), nv.ptr(self.guide), V, E,
                            nv.ptr(self.buckets), nv.stream())
            # destination records (8 bytes per edge, staged into LDS with a start row): a walk's second step without the gather of
            # its node record.  Built when the node records are NOT cache resident -- the default catalogue's 1.7 MB of them are L2
            # hits and the records bought nothing there (r03: 0.419 against 0.413 ms, tools/experiments/) -- i.e. for graphs of more
            # than DEST_INFO_MIN_NODES nodes (BASELINE config 5: 110 M nodes = 880 MB of node records), memory permitting;
            # dest_info = True / False (or PS_GRAPH_DEST_INFO=1 / 0) force it.
            self.dest_info = None
            want = dest_info
            if want is None and os.environ.get("PS_GRAPH_DEST_INFO") in ("0", "1"):
                want = os.environ["PS_GRAPH_DEST_INFO"] == "1"
            if E and want is not False:
                free = torch.cuda.mem_get_info(dev)[0]
                if want is True or (V > self.DEST_INFO_MIN_NODES and E * 8 < free // 4):
                    self.dest_info = torch.empty(2 * E, dtype=torch.int32, device=dev)
                    nv.call("ps_dest_info_build", nv.ptr(self.col), nv.ptr(self.nodeinfo), E, V, nv.ptr(self.dest_info), nv.stream())
            flags = torch.zeros(2, dtype=torch.int64, device=dev)
            nv.call("ps_graph_stats", nv.ptr(self.rowptr), nv.ptr(self.col), E, V, nv.ptr(flags), nv.stream())
            f = flags.tolist()
        self.has_reachable_sink = bool(f[0])
        self.max_degree = int(f[1])
        self.wsorted = wsorted
        self.nbr_sorted = None

    def sorted_neighbors(self):
        """int32[E]: every row's destinations in ascending order, duplicates kept -- what the biased walk (ps_walk_paths_biased)
        searches for "the previous node has an out-edge to x".  One torch sort of (row, col) keys, on the first biased call;
        a sampler with p == q == 1 never builds it."""
        if self.col is None or self.wsorted is None or self.cdf is None:
            gone = [k for k in ("col", "cdf", "wsorted") if getattr(self, k) is None]
            raise ValueError(f"the biased walk (p or q != 1) needs the plain col / cdf / wsorted arrays; {', '.join(gone)} "
                             "dropped by compact() (expand() restores col and cdf from the packed blocks, not wsorted)")
        if self.nbr_sorted is None:
            rows = torch.repeat_interleave(torch.arange(self.V, device=self.device), self.rowptr[1:] - self.rowptr[:-1])
            key = torch.sort(rows * max(self.V, 1) + self.col.to(torch.int64)).values
            self.nbr_sorted = (key - rows * max(self.V, 1)).to(torch.int32).contiguous()
        return self.nbr_sorted

    def compact(self):
        """Drop the plain `col` / `cdf` / `guide` arrays (16 bytes per edge): the walk kernels read the same values from the
        interleaved 128-byte blocks of `packed` (+ `nodeinfo`, `buckets`), which stay.  For graphs that fill the GPU (BASELINE
        config 5: 32 of 162 GB); `expand()` restores them bit for bit.  ps_walk_paths and host-side inspection need the plain
        arrays."""
        if self.packed is None or self.E == 0:
            return self
        self.col = self.cdf = self.guide = None
        self.wsorted = None
        self.nbr_sorted = None               # (the biased walk's table: it cannot run without col / wsorted)
        return self

    def expand(self):
        """Rebuild `col` / `cdf` / `guide` from the packed blocks (exact copies: the blocks hold the same bits)."""
        if self.col is not None or self.E == 0:
            return self
        blk = self.packed.view(-1, 128)
        self.cdf = blk[:, :64].contiguous().view(torch.float64).reshape(-1)[: self.E].contiguous()
        self.col = blk[:, 64:96].contiguous().view(torch.int32).reshape(-1)[: self.E].contiguous()
        self.guide = blk[:, 96:128].contiguous().view(torch.int32).reshape(-1)[: self.E].contiguous()
        return self

    @property
    def walk_flags(self):
        """flags OR-ed into rng_mode of the walk launches (the form of `buckets`)"""
        return nv.PS_WALK_HALF_BUCKETS if self.bucket_bytes == 32 else 0

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.rowptr, self.col, self.cdf, self.nodeinfo, self.guide, self.packed,
                                                         self.buckets, self.dest_info) if t is not None)


def _csr_with_perm(rows, cols, E, V, dev):
    """(rowptr int64[V+1], col int32[E], perm int64[E]) of the edges (rows[e], cols[e]) grouped by row with ps_csr_build's
    stable sort: col = cols in slot order, perm = the position of every slot in the original edge order."""
    rowptr = torch.empty(V + 1, dtype=torch.int64, device=dev)
    col = torch.empty(E, dtype=torch.int32, device=dev)
    order = torch.empty(E, dtype=torch.float64, device=dev)
    ws, wsb = nv.workspace("ps_csr_build_workspace_bytes", dev, E, V)
    # the "weight" channel carries the original edge number (exact in fp32 only below 2^24, so it is passed
    # through the fp64 output by building it in two halves)
    idx = torch.arange(E, device=dev)
    lo16 = (idx & 0xFFFF).to(torch.float32).contiguous()
    hi16 = (idx >> 16).to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        nv.call("ps_csr_build", nv.ptr(rows), nv.ptr(cols), nv.ptr(lo16), E, V, nv.ptr(rowptr), nv.ptr(col),
                nv.ptr(order), nv.ptr(ws), wsb, nv.stream())
        lo_sorted = order.clone()
        nv.call("ps_csr_build", nv.ptr(rows), nv.ptr(cols), nv.ptr(hi16), E, V, nv.ptr(rowptr), nv.ptr(col),
                nv.ptr(order), nv.ptr(ws), wsb, nv.stream())
    return rowptr, col, (order.to(torch.int64) << 16) | lo_sorted.to(torch.int64)


class TargetCSR:
    """Edges grouped by target node (what GraphConv.propagate aggregates over): rowptr / col (= source node) /
    perm (position of every CSR slot in the original edge order, for per-edge weights).  Built with the same
    stable sort as the sampler's adjacency; cached per edge_index tensor by the caller."""

    def __init__(self, edge_index, num_nodes):
        dev = nv.require_gpu() if not edge_index.is_cuda else edge_index.device
        ei = edge_index.to(device=dev, dtype=torch.int64)
        if ei.dim() != 2 or ei.size(0) != 2:
            raise ValueError("edge_index must have shape [2, num_edges]")
        E, V = int(ei.size(1)), int(num_nodes)
        if E:
            # torch / PyG raise on such input (index_add_ / x[src]); the kernels below index rowptr[V+1] and
            # x[num_nodes] with these ids, so they are checked once here (the result is cached by the caller)
            lo, hi = int(ei.min().item()), int(ei.max().item())
            if lo < 0 or hi >= V:
                raise IndexError(f"edge_index holds node id {lo if lo < 0 else hi}, outside [0, {V}) "
                                 "(global ids passed with batch-local features?)")
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        self.V, self.E, self.device = V, E, dev
        self.rowptr, self.col, self.perm = _csr_with_perm(dst, src, E, V, dev)
        self._src, self._dst, self._source = src, dst, None      # the edge rows, kept until source() has grouped them by source

    def source(self):
        """(SourceCSR, index): the same edges grouped by SOURCE node -- rowptr / col (= target node) / perm, from the same
        ps_csr_build with the rows of edge_index not swapped -- and the int64 index that carries a vector from this object's
        slot order to that one's (val_source = val_target[index]; perm is a permutation, so it is one gather).  What the
        gradient of spmm with respect to the features sweeps; built on first use and kept."""
        if self._source is None:
            s = SourceCSR()
            s.V, s.E, s.device = self.V, self.E, self.device
            s.rowptr, s.col, s.perm = _csr_with_perm(self._src, self._dst, self.E, self.V, self.device)
            slot_of_edge = torch.empty_like(self.perm)
            slot_of_edge[self.perm] = torch.arange(self.E, device=self.device)
            self._source = (s, slot_of_edge[s.perm])
            self._src = self._dst = None
        return self._source


class SourceCSR:
    """The edges of a TargetCSR grouped by source node (TargetCSR.source): V, E, device, rowptr, col (= target node), perm."""


def spmm_csr(tcsr, x, val=None):
    """out[r] = sum_e val[e] * x[col[e]] over row r of a TargetCSR (val in CSR slot order)."""
    x = x.contiguous()
    out = torch.empty((tcsr.V, x.size(1)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nv.call("ps_spmm_csr", nv.ptr(tcsr.rowptr), nv.ptr(tcsr.col), nv.ptr(val), nv.ptr(x), x.size(0), x.size(1), tcsr.V, tcsr.E,
                nv.ptr(out), nv.stream())
    return out


def spmm_csr_exact(csr, x, val=None):
    """spmm_csr without atomics (ps_spmm_csr_exact): every output bit is a function of the inputs.  csr: a TargetCSR or the
    SourceCSR of one; x fp32 [N, H] and val fp32 [E] (slot order) contiguous."""
    N, H = int(x.size(0)), int(x.size(1))
    out = torch.empty((csr.V, H), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws, nbytes = nv.workspace("ps_spmm_csr_exact_workspace_bytes", x.device, csr.E, H)
        nv.call("ps_spmm_csr_exact", nv.ptr(csr.rowptr), nv.ptr(csr.col), nv.ptr(val), nv.ptr(x), N, H, csr.V, csr.E, nv.ptr(out),
                nv.ptr(ws), nbytes, nv.stream())
    return out


def sddmm_csr(csr, x, g):
    """d[e] = g[r] . x[col[e]] for every slot e of row r (ps_sddmm_csr): the gradient of spmm_csr_exact's val.  x fp32 [N, H],
    g fp32 [V, H] contiguous."""
    d = torch.empty(csr.E, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nv.call("ps_sddmm_csr", nv.ptr(csr.rowptr), nv.ptr(csr.col), nv.ptr(x), int(x.size(0)), nv.ptr(g), csr.V, int(x.size(1)),
                csr.E, nv.ptr(d), nv.stream())
    return d


def use_hip_grad(*tensors):
    """sampling.grad_method == "hip" and every tensor is CUDA fp32: the one switch of every HIP backward (read here, at call
    time: this module does not import sampling when it is loaded)."""
    from . import sampling
    return sampling._use_hip_grad(*tensors)


def _slot_rows(csr):
    """int64 [E]: the row of every slot (a search per slot: nothing waits for the host)"""
    return torch.searchsorted(csr.rowptr, torch.arange(csr.E, device=csr.rowptr.device), right=True) - 1


def spmm_torch(tcsr, x, val=None):
    """spmm_csr as a differentiable torch expression over an [E, H] tensor (grad_method "torch", N != V, other dtypes)"""
    msg = x[tcsr.col.long().to(x.device)]
    if val is not None:
        msg = msg * val.view(-1, 1)
    return torch.zeros((tcsr.V, x.size(1)), dtype=msg.dtype, device=x.device).index_add_(0, _slot_rows(tcsr).to(x.device), msg)


class SpmmFn(torch.autograd.Function):
    """Differentiable ps_spmm_csr_exact over a TargetCSR: out[r] = sum over the slots e of row r of val[e] x[col[e]].
    dx[s] = sum over the edges leaving s of val[e] g[target(e)]: the same kernel over the source-grouped CSR with g as the feature
    matrix and val carried to that slot order; dval[e] = g[r] . x[col[e]]: ps_sddmm_csr, computed (and x saved for it) only when
    val needs a gradient.  No float atomics and no [E, H] tensor in either direction: the same bits on every run."""

    @staticmethod
    def forward(ctx, tcsr, x, val):
        ctx.tcsr = tcsr
        ctx.save_for_backward(val, x if val is not None and ctx.needs_input_grad[2] else None)
        return spmm_csr_exact(tcsr, x.contiguous(), None if val is None else val.contiguous())

    @staticmethod
    def backward(ctx, grad_out):
        val, x = ctx.saved_tensors
        tcsr = ctx.tcsr
        need_x, need_val = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        # a backward that is itself recorded (create_graph) keeps the differentiable torch code
        if not use_hip_grad(grad_out) or (torch.is_grad_enabled() and grad_out.requires_grad):
            rows, cols = _slot_rows(tcsr), tcsr.col.long()
            dx = dval = None
            if need_x:
                msg = grad_out[rows] if val is None else grad_out[rows] * val.view(-1, 1)
                dx = torch.zeros_like(grad_out).index_add_(0, cols, msg)
            if need_val:
                dval = (grad_out[rows] * x[cols]).sum(dim=1)
            return None, dx, dval
        g = grad_out.contiguous()                                     # out.sum().backward() hands over a stride-0 tensor
        dx = dval = None
        if need_x:
            scsr, index = tcsr.source()
            dx = spmm_csr_exact(scsr, g, None if val is None else val[index])
        if need_val:
            dval = sddmm_csr(tcsr, x.contiguous(), g)
        return None, dx, dval


def spmm(tcsr, x, val=None):
    """spmm_csr_exact that stays on the autograd tape when `x` or `val` needs a gradient.  The torch expression serves where the
    kernels do not: sampling.grad_method == "torch", tensors that are not CUDA fp32, x with another row count than the graph."""
    floats = (x,) if val is None else (x, val)
    if not use_hip_grad(*floats) or int(x.size(0)) != tcsr.V:
        return spmm_torch(tcsr, x, val)
    if torch.is_grad_enabled() and any(t.requires_grad for t in floats):
        return SpmmFn.apply(tcsr, x, val)
    return spmm_csr_exact(tcsr, x.contiguous(), None if val is None else val.contiguous())
