"""Personalized-PageRank neighbourhoods over a DeviceGraph (the kernels behind RandomWalkSampler.compute_ppr_matrix /
precompute_top_neighbors / ppr_batch; reference utils/random_walk.py:144-229).

`PPRGraph` is the per-graph part, built once and cached on the DeviceGraph: the push shares (ps_ppr_shares), the in-edges of
every node in the order the reference's sweep adds them (csrc/ppr_push.hip) and the level lists.  `ppr_scores` / `ppr_topk` run
the sweeps for any number of sources, a chunk of columns at a time."""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import native as nv
from .sampling import WeightedBatch

BYTES_PER_STATE = 8 * 4            # per (node, source column): score, two push buffers, the source-major copy


class PPRGraph:
    """in_rowptr int64[V+1] / in_src int32 / in_share fp64: the edges u -> v grouped by v, a stable sort of the out-CSR's slots
    (sources ascending, multi-edges in adjacency order) with the sources u > v ahead of u < v and self-loops dropped;
    level_nodes int32[V] + level_ptr (host): nodes grouped by level(v) = 1 + max level(u) over the in-neighbours u < v."""

    def __init__(self, graph):
        if graph.col is None or graph.wsorted is None:
            raise nv.NativeError("PPR needs the plain CSR arrays: call DeviceGraph.expand() and keep wsorted (not compact())")
        dev, V, E = graph.device, graph.V, graph.E
        self.graph, self.device, self.V = graph, dev, V
        with torch.cuda.device(dev):
            share = torch.empty(E, dtype=torch.float64, device=dev)
            nv.call("ps_ppr_shares", nv.ptr(graph.rowptr), nv.ptr(graph.wsorted), V, nv.ptr(share), nv.stream())
            self.share = share
            src = torch.repeat_interleave(torch.arange(V, device=dev), graph.rowptr[1:] - graph.rowptr[:-1])
            dst = graph.col.to(torch.int64)
            keep = torch.nonzero(src != dst).reshape(-1)
            src, dst = src[keep], dst[keep]
            # per target: u > v first, then u < v; a stable sort keeps the slot order (= ascending u) inside both parts
            order = torch.sort(dst * 2 + (src < dst).to(torch.int64), stable=True)[1]
            self.in_src = src[order].to(torch.int32).contiguous()
            self.in_share = share[keep[order]].contiguous()
            self.in_rowptr = torch.zeros(V + 1, dtype=torch.int64, device=dev)
            if V:
                self.in_rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=V), 0)
            # levels: the longest chain of ascending edges that ends in v, by relaxation (one pass per level)
            lower = src < dst
            ls, ld = src[lower], dst[lower]
            level = torch.zeros(V, dtype=torch.int64, device=dev)
            while ls.numel():
                nxt = level.scatter_reduce(0, ld, level[ls] + 1, "amax")
                if torch.equal(nxt, level):
                    break
                level = nxt
            self.level_nodes = torch.sort(level, stable=True)[1].to(torch.int32).contiguous()
            counts = torch.bincount(level).cpu().numpy() if V else np.zeros(1, dtype=np.int64)
        self.n_levels = int(counts.size)
        self.level_ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))


def ppr_graph(graph):
    """the PPRGraph of a DeviceGraph, built on first use"""
    pg = getattr(graph, "_ppr_graph", None)
    if pg is None:
        pg = graph._ppr_graph = PPRGraph(graph)
    return pg


def _check(alpha, sweeps):
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError("alpha must lie in (0, 1)")
    if int(sweeps) < 0:
        raise ValueError("num_iterations must not be negative")


def _sources(sources, device):
    if isinstance(sources, torch.Tensor):
        sources = sources.detach().cpu().numpy()
    a = np.asarray(sources, dtype=np.int64).reshape(-1)
    if a.size and a.min() < 0:
        raise IndexError("negative source node")
    return a, torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _chunk(S, Vp, device, source_chunk):
    if source_chunk is not None:
        c = int(source_chunk)
        if c < 64 or c % 64:
            raise ValueError("source_chunk must be a positive multiple of 64")
        return c
    free = torch.cuda.mem_get_info(device)[0]
    fit = max(64, (free // 2) // max(1, Vp * BYTES_PER_STATE) // 64 * 64)
    return int(min(fit, -(-S // 64) * 64))


def _push_chunks(graph, sources, alpha, sweeps, source_chunk, skip_rows):
    """yields (lo, n, score_t fp64[n, Vp] source-major, the chunk's sources int64[n] on the device) per chunk of source columns"""
    _check(alpha, sweeps)
    pg = ppr_graph(graph)
    dev = pg.device
    host, src = _sources(sources, dev)
    S = int(host.size)
    Vp = max(pg.V, int(host.max()) + 1) if S else pg.V
    alpha_bits = struct.unpack("<Q", struct.pack("<d", float(alpha)))[0]
    flags = 0 if skip_rows else nv.PS_PPR_NO_SKIP
    chunk = _chunk(S, Vp, dev, source_chunk) if S else 64
    with torch.cuda.device(dev):
        for lo in range(0, S, chunk):
            n = min(chunk, S - lo)
            Sc = -(-n // 64) * 64
            score = torch.empty((Vp, Sc), dtype=torch.float64, device=dev)
            ws, ws_bytes = nv.workspace("ps_ppr_push_workspace_bytes", dev, Vp, n)
            nv.call("ps_ppr_push", nv.ptr(pg.in_rowptr), nv.ptr(pg.in_src), nv.ptr(pg.in_share), pg.V, Vp, nv.ptr(pg.level_nodes),
                    pg.level_ptr.ctypes.data, pg.n_levels, nv.ptr(src[lo:lo + n]), n, alpha_bits, int(sweeps), flags,
                    nv.ptr(score), nv.ptr(ws), ws_bytes, nv.stream())
            del ws
            yield lo, n, score[:, :n].t().contiguous(), src[lo:lo + n]


def ppr_scores(graph, sources, alpha=0.15, sweeps=10, source_chunk=None, skip_rows=True):
    """fp64[S, V'] on the device: row i = the reference's `ppr` vector of sources[i] after `sweeps` push sweeps
    (utils/random_walk.py:163-188), V' = max(V, max(sources) + 1); a source >= V is a node without edges.  Sources run in
    chunks of columns sized from free memory (multiples of 64); `source_chunk` sets the chunk size."""
    rows = [t for _, _, t, _ in _push_chunks(graph, sources, alpha, sweeps, source_chunk, skip_rows)]
    if not rows:
        return torch.zeros((0, graph.V), dtype=torch.float64, device=graph.device)
    return rows[0] if len(rows) == 1 else torch.cat(rows, 0)


def ppr_topk(graph, sources, k=10, alpha=0.15, sweeps=10, max_target=None, source_chunk=None, skip_rows=True):
    """-> WeightedBatch: per source the k best targets with a positive score, score descending, ties to the smaller id, and
    weights = score / their left-to-right sum (utils/random_walk.py:213-227); `.scores` holds the raw scores.  Only targets
    below `max_target` compete when it is given."""
    k = int(k)
    if k < 1:
        raise ValueError("num_neighbors must be at least 1")
    dev = graph.device
    S = int(len(sources)) if not isinstance(sources, torch.Tensor) else int(sources.numel())
    ids = torch.empty((S, k), dtype=torch.int32, device=dev)
    scores = torch.empty((S, k), dtype=torch.float64, device=dev)
    wts = torch.empty((S, k), dtype=torch.float64, device=dev)
    nvalid = torch.empty(S, dtype=torch.int32, device=dev)
    mt = -1 if max_target is None else int(max_target)
    if max_target is not None and mt < 0:
        raise ValueError("max_target must not be negative")
    for lo, n, rows, _ in _push_chunks(graph, sources, alpha, sweeps, source_chunk, skip_rows):
        Vp = int(rows.size(1))
        with torch.cuda.device(dev):
            nv.call("ps_ppr_topk", nv.ptr(rows), n, Vp, Vp, mt, k, nv.ptr(ids[lo:lo + n]), nv.ptr(scores[lo:lo + n]),
                    nv.ptr(wts[lo:lo + n]), nv.ptr(nvalid[lo:lo + n]), nv.stream())
    batch = WeightedBatch(ids, wts, nvalid)
    batch.scores = scores
    return batch


def ppr_rank_window(graph, sources, lo, hi, *, n=0, uniforms=None, alpha=0.15, sweeps=10, max_target=None, skip_self=True,
                    source_chunk=None, skip_rows=True):
    """-> (window int32[S, hi - lo], nwin int32[S], picks int32[S, n] or None) on the device: per source the targets whose rank
    in ppr_topk's order (score descending, ties to the smaller id, 0-based) lies in [lo, hi), in ascending id order with -1
    pads, and with n > 0 a Floyd subset of them drawn from `uniforms` fp64[S, n] (ps_rank_window, include/pinsage_hip.h).  Only
    targets below `max_target` compete when it is given; skip_self leaves the source itself out of its own ranking."""
    lo, hi, n = int(lo), int(hi), int(n)
    if lo < 0 or hi <= lo:
        raise ValueError("the rank window needs 0 <= lo < hi")
    if hi - lo > nv.lib().ps_rank_window_max():
        raise ValueError(f"the rank window holds at most {nv.lib().ps_rank_window_max()} ranks")
    if n < 0:
        raise ValueError("n must not be negative")
    dev = graph.device
    S = int(len(sources)) if not isinstance(sources, torch.Tensor) else int(sources.numel())
    u = None
    if n > 0:
        if uniforms is None or tuple(np.shape(uniforms)) != (S, n):
            raise ValueError(f"n = {n} picks need uniforms of shape [{S}, {n}]")
        u = uniforms if isinstance(uniforms, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64))
        u = u.to(device=dev, dtype=torch.float64).contiguous()
    mt = -1 if max_target is None else int(max_target)
    if max_target is not None and mt < 0:
        raise ValueError("max_target must not be negative")
    window = torch.empty((S, hi - lo), dtype=torch.int32, device=dev)
    nwin = torch.empty(S, dtype=torch.int32, device=dev)
    picks = torch.empty((S, n), dtype=torch.int32, device=dev) if n > 0 else None
    for c0, c, rows, src in _push_chunks(graph, sources, alpha, sweeps, source_chunk, skip_rows):
        Vp = int(rows.size(1))
        with torch.cuda.device(dev):
            nv.call("ps_rank_window", nv.ptr(rows), c, Vp, Vp, mt, nv.ptr(src if skip_self else None), lo, hi,
                    nv.ptr(u[c0:c0 + c] if n > 0 else None), n, nv.ptr(window[c0:c0 + c]), nv.ptr(nwin[c0:c0 + c]),
                    nv.ptr(picks[c0:c0 + c] if n > 0 else None), nv.stream())
    return window, nwin, picks
