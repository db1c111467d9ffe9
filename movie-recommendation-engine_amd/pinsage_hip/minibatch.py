"""Minibatch blocks: the K-hop sampled neighbourhood of a batch of items, layer by layer (PinSage paper, Algorithm 2).

`frontier` binds ps_frontier_build (csrc/frontier.hip): seeds + a [B, T] neighbour table -> the node set "seeds first, then every
other kept id once, ascending" and the table renumbered into that set.  A `Block` is one layer of the expansion: its destination
nodes are a PREFIX of its source nodes, so the layer's "self" rows are the slice h[:n_dst] -- no gather forward, no scatter
backward.  RandomWalkSampler.sample_blocks builds the blocks top-down, PinSage.forward_blocks walks them bottom-up."""
from __future__ import annotations

import numpy as np
import torch

from . import native as nv


def frontier(seeds, ids, nvalid, limit):
    """(frontier[:count], local) of ps_frontier_build.  seeds: int32 [S] device tensor of distinct ids in [0, limit), or None
    (S = 0); ids int32 [B, T] / nvalid int32 [B]: a neighbour table on the same device, or None / None (B = 0: `local` is then
    an empty [0, 1] tensor).  Device tensors in and out; the one host read is `count`."""
    given = seeds if seeds is not None else ids
    if given is None:
        raise ValueError("frontier needs seeds or a neighbour table")
    dev = given.device
    S = 0 if seeds is None else int(seeds.numel())
    B, T = (0, 1) if ids is None else (int(ids.size(0)), int(ids.size(1)))
    for name, t in (("seeds", seeds), ("ids", ids), ("nvalid", nvalid)):
        if t is not None and (t.dtype != torch.int32 or t.device != dev):
            raise TypeError(f"{name} must be an int32 tensor on {dev}")
    if (ids is None) != (nvalid is None) or (ids is not None and (ids.dim() != 2 or nvalid.numel() != B)):
        raise ValueError("ids [B, T] and nvalid [B]: both or neither")
    limit = int(limit)
    if limit < 1 or limit >= 2 ** 31 or T < 1 or B * T >= 2 ** 31 or S + min(B * T, limit) >= 2 ** 31:
        raise ValueError(f"frontier: limit {limit}, S {S}, B {B}, T {T} are outside ps_frontier_build's range")
    if seeds is not None:
        seeds = seeds.reshape(-1).contiguous()
    if ids is not None:
        ids, nvalid = ids.contiguous(), nvalid.reshape(-1).contiguous()
    out = torch.empty(S + min(B * T, limit), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    local = torch.empty((B, T), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = nv.workspace("ps_frontier_workspace_bytes", dev, limit, S, B, T)
        nv.call("ps_frontier_build", nv.ptr(seeds), S, nv.ptr(ids), nv.ptr(nvalid), B, T, limit, nv.ptr(out), nv.ptr(count),
                nv.ptr(local), nv.ptr(ws), nbytes, nv.stream())
    return out[:int(count.item())], local


class Block:
    """One layer of a minibatch: the layer reads the rows of `src_nodes` and writes the rows of its first `n_dst` entries.

    src_nodes  int32 [n_src]: global ids; the destination nodes are src_nodes[:n_dst]
    ids        int32 [n_dst, T]: every destination's neighbour list as positions in src_nodes, -1 where the slot is not kept
    counts     int32 [n_dst, T] visit counts (walks), or None
    wts        [n_dst, T] weights (personalized PageRank), or None
    nvalid     int32 [n_dst]"""

    __slots__ = ("src_nodes", "n_dst", "ids", "counts", "wts", "nvalid")

    def __init__(self, src_nodes, n_dst, ids, nvalid, counts=None, wts=None):
        if (counts is None) == (wts is None):
            raise ValueError("a Block carries counts or wts, not both")
        self.src_nodes, self.n_dst, self.ids, self.nvalid, self.counts, self.wts = src_nodes, int(n_dst), ids, nvalid, counts, wts

    @property
    def n_src(self):
        return int(self.src_nodes.numel())

    @property
    def dst_nodes(self):
        return self.src_nodes[:self.n_dst]

    def __repr__(self):
        return f"Block(n_src={self.n_src}, n_dst={self.n_dst}, T={int(self.ids.size(1))}, {'counts' if self.wts is None else 'wts'})"


def unique_seeds(seeds, n_items, device):
    """(distinct seeds ascending int32 [n], inverse int64 [len(seeds)]) on `device`: ps_frontier_build with S = 0 over the seeds
    as a [len, 1] table.  A seed outside [0, n_items) raises ValueError (the one host read besides the count)."""
    if isinstance(seeds, torch.Tensor):
        s = seeds.reshape(-1).to(device=device, dtype=torch.int64)
    else:
        s = torch.from_numpy(np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1))).to(device)
    if s.numel() == 0:
        raise ValueError("sample_blocks needs at least one seed")
    lo, hi = int(s.min().item()), int(s.max().item())
    if lo < 0 or hi >= n_items:
        raise ValueError(f"seeds must be item ids in [0, {n_items}); got {lo if lo < 0 else hi}")
    table = s.to(torch.int32).view(-1, 1).contiguous()
    uniq, local = frontier(None, table, torch.ones(table.size(0), dtype=torch.int32, device=device), n_items)
    return uniq, local.view(-1).long()


def build_blocks(nodes, sample_layer, layers, n_items):
    """The blocks of `layers` layers over the distinct seeds `nodes` (int32 device tensor), widest first.  sample_layer(i, nodes)
    -> (ids, nvalid, counts, wts) is layer i's neighbour table of `nodes`; it is called for i = layers - 1 down to 0, each time
    with the source nodes of the block above."""
    blocks = [None] * layers
    for i in range(layers - 1, -1, -1):
        ids, nvalid, counts, wts = sample_layer(i, nodes)
        src, local = frontier(nodes, ids, nvalid, n_items)
        blocks[i] = Block(src, nodes.numel(), local, nvalid, counts=counts, wts=wts)
        nodes = src
    return blocks
