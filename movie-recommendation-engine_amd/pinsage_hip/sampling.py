"""Tensor-native sampling ops over a DeviceGraph (the kernels behind RandomWalkSampler).

`NeighborBatch` is the device-resident result ([B,T] ids / visit counts, [B] nvalid), `WeightedBatch` its
counterpart with fp64 weights (personalized PageRank);
`LazyNeighborList` is the python list-of-lists view the reference API returns
(utils/random_walk.py:119-142), materialised only when python code actually looks at it."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import native as nv


class NeighborBatch:
    """ids int32[B,T] (-1 pad), counts int32[B,T] (0 pad), nvalid int32[B] on the device."""

    def __init__(self, ids, counts, nvalid):
        self.ids, self.counts, self.nvalid = ids, counts, nvalid
        self._host = None

    @property
    def B(self):
        return int(self.ids.size(0))

    @property
    def T(self):
        return int(self.ids.size(1))

    def host(self):
        """(ids int64, counts int32, nvalid int32, weights fp64) as numpy; weights = count / sum(top
        counts) in fp64 exactly like python's int/int (utils/random_walk.py:113-115)."""
        if self._host is None:
            ids = self.ids.cpu().numpy().astype(np.int64)
            counts = self.counts.cpu().numpy()
            nvalid = self.nvalid.cpu().numpy()
            tot = counts.sum(axis=1, dtype=np.int64)
            w = counts.astype(np.float64) / np.maximum(tot, 1)[:, None].astype(np.float64)
            self._host = (ids, counts, nvalid, w)
        return self._host

    def to_lists(self):
        ids, counts, nvalid, w = self.host()
        nb = [list(ids[i, :nvalid[i]]) for i in range(ids.shape[0])]          # np.int64 scalars
        wt = [w[i, :nvalid[i]].tolist() for i in range(ids.shape[0])]          # python floats
        return nb, wt


class WeightedBatch:
    """ids int32[B,T] (-1 pad), wts fp64[B,T] (0 pad), nvalid int32[B] on the device: neighbourhoods that come with their
    weights (personalized PageRank, pinsage_hip/ppr.py) instead of visit counts.  Same B / T / to_lists() as NeighborBatch,
    so LazyNeighborList serves both.  `scores` (fp64[B,T], optional): the values the weights were normalised from."""

    def __init__(self, ids, wts, nvalid):
        self.ids, self.wts, self.nvalid = ids, wts, nvalid
        self.scores = None
        self._host = None

    @property
    def B(self):
        return int(self.ids.size(0))

    @property
    def T(self):
        return int(self.ids.size(1))

    def host(self):
        """(ids int64, wts fp64, nvalid int32) as numpy"""
        if self._host is None:
            self._host = (self.ids.cpu().numpy().astype(np.int64), self.wts.cpu().numpy(), self.nvalid.cpu().numpy())
        return self._host

    def to_lists(self):
        ids, w, nvalid = self.host()
        nb = [list(ids[i, :nvalid[i]]) for i in range(ids.shape[0])]          # np.int64 scalars
        wt = [w[i, :nvalid[i]].tolist() for i in range(ids.shape[0])]          # python floats
        return nb, wt


class LazyNeighborList(list):
    """A real `list` (isinstance checks in the reference pass) whose items are produced from the
    device batch on first python-level access.  Our own kernels read `.batch` and never touch it.
    Until then the C-level list holds `None` placeholders of the right length, so consumers that bypass the python
    protocol (PySequence_Fast: `torch.tensor(lst)`, `np.asarray(lst)` on some paths) fail loudly on a None instead of
    silently seeing an empty list; `.materialize()` (or any python-level access) fills it."""

    EAGER_BELOW = 4096

    def __init__(self, batch, kind: str):
        super().__init__()
        self.batch = batch
        self.kind = kind
        self._done = False
        if batch.B <= self.EAGER_BELOW:       # small batches: a plain, fully populated list (C-level consumers too)
            self._fill()
        else:
            super().extend([None] * batch.B)

    def _fill(self):
        if not self._done:
            self._done = True
            nb, wt = self.batch.to_lists()
            list.__setitem__(self, slice(None), nb if self.kind == "ids" else wt)

    def materialize(self):
        """fill the list now (for code that hands it to C-level consumers)"""
        self._fill()
        return self

    def __len__(self):
        return self.batch.B

    def __iter__(self):
        self._fill()
        return super().__iter__()

    def __getitem__(self, i):
        self._fill()
        return super().__getitem__(i)

    def __eq__(self, other):
        self._fill()
        return super().__eq__(other)

    def __repr__(self):
        self._fill()
        return super().__repr__()

    def __bool__(self):
        return self.batch.B > 0

    def __reduce__(self):
        self._fill()
        return (list, (list(super().__iter__()),))


def _nodes_tensor(nodes, device, num_nodes):
    """int64 device tensor of start nodes.  Host inputs (lists / numpy / CPU tensors) are range-checked
    here like the reference's `adj_list[node]` (utils/random_walk.py:66 -> IndexError); tensors already
    on the device are not synchronised on: the kernels treat out-of-range ids as isolated nodes."""
    if isinstance(nodes, torch.Tensor) and nodes.is_cuda:
        return nodes.to(device=device, dtype=torch.int64).reshape(-1).contiguous()
    a = nodes.numpy() if isinstance(nodes, torch.Tensor) else np.asarray(nodes)
    a = a.astype(np.int64, copy=False).reshape(-1)
    if a.size and (a.min() < -num_nodes or a.max() >= num_nodes):
        raise IndexError("list index out of range")
    if a.size and a.min() < 0:
        a = np.where(a < 0, a + num_nodes, a)            # python negative indexing into adj_list
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def draw_numpy_uniforms(n, device, defer_state=False, raw=False, ranges=None):
    """n doubles of the process-global legacy numpy stream, exactly what n sequential
    `np.random.choice(..., p=...)` calls consume (utils/random_walk.py:79), staged to HBM.
    defer_state: see dense.mt19937_random_sample(advance='defer').  raw=True: the caller can consume the stream as raw
    MT19937 words (PS_RNG_STREAM_RAW); returns (tensor, is_raw) -- short requests are drawn on the host as doubles.
    ranges (raw): the runs of uniform indices the caller reads (dense.mt19937_random_sample); the rest stays unwritten."""
    if n >= (1 << 17):
        from . import dense                    # same stream, generated on the device (jump-ahead chunks)
        t = dense.mt19937_random_sample(int(n), device, advance="defer" if defer_state else True, raw=raw, ranges=ranges if raw else None)
        return (t, True) if raw else t
    if raw:
        return draw_numpy_uniforms(n, device, defer_state), False
    u = np.random.random_sample(int(n))
    t = torch.from_numpy(u)
    if n:
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def sink_walk_offsets(graph, starts, W, L, uniforms):
    """Stream position of every walk, int64[B * W], on a graph with REACHABLE SINKS, plus the number of uniforms the batch
    consumes.  The reference breaks a walk at a node without out-edges before drawing (utils/random_walk.py:65-69), so a walk
    consumes between 0 and L uniforms and walk j starts at the running count of uniforms consumed by every earlier walk:
    off_j = sum_{i<j} steps_i, steps_j = f_j(off_j).  That recurrence has exactly one solution, and it is found in parallel as a
    fixpoint: walk all B * W walks from guessed positions (ps_walk_paths), count the steps they took, prefix-sum, repeat until
    the counts reproduce themselves.  Every pass makes at least one more leading walk final, so it terminates; where the
    number of steps is decided by the graph rather than by the draw (e.g. every walk from a user lands on an item that is a
    sink) two or three passes are enough.  Exact, slower than the sink-free path, and only taken by graphs that need it."""
    dev = graph.device
    B = int(starts.numel())
    walks = starts.repeat_interleave(W).contiguous()
    ok = (starts >= 0) & (starts < graph.V)
    deg = torch.zeros(B, dtype=torch.int64, device=dev)
    deg[ok] = graph.rowptr[starts[ok] + 1] - graph.rowptr[starts[ok]]
    steps = ((deg > 0).to(torch.int64) * L).repeat_interleave(W)
    paths = torch.empty((B * W, L), dtype=torch.int32, device=dev)
    off = torch.zeros(B * W, dtype=torch.int64, device=dev)
    for _ in range(B * W + 2):
        off = (torch.cumsum(steps, 0) - steps).contiguous()
        if B * W == 0:
            break
        nv.call("ps_walk_paths", nv.ptr(graph.rowptr), nv.ptr(graph.col), nv.ptr(graph.cdf), graph.V, nv.ptr(walks), B * W, L,
                nv.PS_RNG_STREAM, nv.ptr(uniforms), nv.ptr(off), 0, 0, 0, nv.ptr(graph.nodeinfo), nv.ptr(graph.guide),
                nv.ptr(paths), nv.stream())
        took = (paths >= 0).sum(dim=1)
        if torch.equal(took, steps):
            return off, int(steps.sum().item())
        steps = took
    return off, int(steps.sum().item())


def _sink_stream(graph, starts, W, L, uniforms=None):
    """(uniforms on the device, per-walk offsets) for a batch on a graph with reachable sinks; draws from np.random what the
    reference would (at most one uniform per step; the global state ends exactly where the reference leaves it)."""
    dev = graph.device
    B = int(starts.numel())
    given = uniforms is not None
    if not given:
        state = np.random.get_state()
        host = np.random.random_sample(B * W * L + 1)          # the most the batch can consume (+1: never an empty buffer)
        uniforms = torch.from_numpy(host).to(dev)
    off, total = sink_walk_offsets(graph, starts, W, L, uniforms)
    if not given:
        np.random.set_state(state)
        np.random.random_sample(total)                           # advance the global stream by what was really consumed
    return uniforms, off


def _uniform_offsets(graph, starts, W, L):
    """ps_uniform_offsets: (stream position of every start node on a sink-free graph int64[B], uniforms consumed int64[1])"""
    dev = graph.device
    total = torch.empty(1, dtype=torch.int64, device=dev)
    uoff = torch.empty(starts.numel(), dtype=torch.int64, device=dev)
    nv.call("ps_uniform_offsets", nv.ptr(graph.rowptr), graph.V, nv.ptr(starts), starts.numel(), W, L, nv.ptr(uoff), nv.ptr(total),
            nv.stream())
    return uoff, total


def _stream_plan(graph, starts, W, L, rng, uniforms=None, stream_nodes=None):
    """(uniforms, uoff, mode) of W walks of L steps from every node of `starts` (device int64): nothing for rng='philox'; for
    rng='numpy' the global stream's uniforms (drawn here unless given) and one position per start node (PS_RNG_STREAM) or, on a
    graph with reachable sinks, per walk (PS_RNG_STREAM_WALKS).  stream_nodes = (all nodes, lo): `starts` is the slice from `lo`
    of that logical batch; positions and uniforms are those of all of it."""
    if rng == "philox":
        return None, None, nv.PS_RNG_PHILOX
    if rng != "numpy":
        raise ValueError("rng must be 'numpy' or 'philox'")
    dev = graph.device
    B = int(starts.numel())
    all_t, lo = starts, 0
    if stream_nodes is not None:
        all_t, lo = _nodes_tensor(stream_nodes[0], dev, graph.V), stream_nodes[1]
    if graph.has_reachable_sink:
        # data-dependent RNG consumption (utils/random_walk.py:65-69): per-walk stream positions by fixpoint
        uniforms, uoff = _sink_stream(graph, all_t, W, L, uniforms)
        if stream_nodes is not None:
            uoff = uoff[lo * W:(lo + B) * W].contiguous()
        return uniforms, uoff, nv.PS_RNG_STREAM_WALKS
    uoff, total = _uniform_offsets(graph, all_t, W, L)
    if stream_nodes is not None:
        uoff = uoff[lo:lo + B].contiguous()
    if uniforms is None:
        uniforms = draw_numpy_uniforms(int(total.item()), dev)
    return uniforms, uoff, nv.PS_RNG_STREAM


def is_biased(p, q):
    """does (p, q) ask for the second-order (node2vec) walk?  p == q == 1 is the reference's first-order walk and runs the kernels it always ran"""
    return not (p == 1.0 and q == 1.0)


def check_bias(p, q):
    """(1 / p, 1 / q) as python floats; p (return) and q (in-out) must be finite and greater than 0, and so must their inverses"""
    try:
        p, q = float(p), float(q)
        ok = math.isfinite(p) and math.isfinite(q) and p > 0 and q > 0 and math.isfinite(1.0 / p) and math.isfinite(1.0 / q)
    except (TypeError, ValueError, ZeroDivisionError):
        ok = False
    if not ok:
        raise ValueError(f"p and q must be finite and greater than 0, got p={p!r}, q={q!r}")
    return 1.0 / p, 1.0 / q


def _no_biased_sinks(graph, rng):
    if rng == "numpy" and graph.has_reachable_sink:
        raise NotImplementedError("biased walks (p or q != 1) with rng='numpy' on a graph with reachable sinks are not implemented: "
                                  "a walk that stops early shifts every later stream position.  Use rng='philox' there.")


def _biased_paths(graph, walks, L, mode, uniforms, uoff, seed, call, walk_mod, p, q):
    """ps_walk_paths_biased over `walks` (int64 start node per walk) -> int32[len(walks), L]"""
    dev = graph.device
    inv_p, inv_q = check_bias(p, q)
    nbr = graph.sorted_neighbors()
    bias = torch.tensor([inv_p, inv_q], dtype=torch.float64, device=dev)
    n = int(walks.numel())
    paths = torch.empty((n, L), dtype=torch.int32, device=dev)
    nv.call("ps_walk_paths_biased", nv.ptr(graph.rowptr), nv.ptr(graph.col), nv.ptr(graph.wsorted), nv.ptr(graph.cdf), nv.ptr(nbr),
            graph.V, nv.ptr(walks), n, L, mode, nv.ptr(uniforms), nv.ptr(uoff), seed & (2 ** 64 - 1), call, walk_mod, nv.ptr(bias),
            nv.ptr(paths), nv.stream())
    return paths


def paths_topk_max_entries():
    """the most entries (W * L) per start node that ps_paths_topk counts"""
    return int(nv.lib().ps_paths_topk_max_entries())


def paths_topk(paths, T):
    """NeighborBatch of given paths int32[B, n] (n = W * L, walk-major, -1 entries skipped): ps_walk_sample's counting and cut"""
    B, n = int(paths.size(0)), int(paths.size(1))
    dev = paths.device
    ids = torch.empty((B, T), dtype=torch.int32, device=dev)
    counts = torch.empty((B, T), dtype=torch.int32, device=dev)
    nvalid = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nv.call("ps_paths_topk", nv.ptr(paths), B, n, T, nv.ptr(ids), nv.ptr(counts), nv.ptr(nvalid), nv.stream())
    return NeighborBatch(ids, counts, nvalid)


def walk_sample(graph, nodes, T, W=100, L=2, rng="numpy", seed=0, call=0, uniforms=None, use_guide=True, use_packed=True, use_buckets=True,
                stream_nodes=None, use_dest=True, p=1.0, q=1.0):
    """batch_sample_neighbors on the device.  rng='numpy': the global numpy stream (bit-exact with
    the reference; graphs with reachable sinks take the per-walk stream positions of sink_walk_offsets);
    rng='philox': counter-based.
    `uniforms` (device fp64) overrides the numpy draw (tests).  `stream_nodes` (rng='numpy' only): the complete
    start-node sequence of the logical batch this call is a contiguous slice of (item shards): the stream offsets
    are computed over all of them and the whole batch's uniforms are drawn, so the ids/counts equal the matching
    rows of the unsharded call and the global np.random state ends where the unsharded call leaves it.
    p / q other than 1 (node2vec's return and in-out parameters): the W walks of every start node are walked by
    ps_walk_paths_biased, at the stream positions / Philox counters the first-order kernel gives them, and counted by
    ps_paths_topk; the accelerator switches (use_*) do not apply.  p == q == 1 changes nothing."""
    dev = graph.device
    biased = is_biased(p, q)
    if biased:
        check_bias(p, q)
        _no_biased_sinks(graph, rng)
        if W * L > paths_topk_max_entries():
            raise ValueError(f"a biased sampler (p or q != 1) counts at most {paths_topk_max_entries()} visits per start node "
                             f"(ps_paths_topk); num_walks * walk_length = {W} * {L} = {W * L}")
    starts = _nodes_tensor(nodes, dev, graph.V)
    B = int(starts.numel())
    with torch.cuda.device(dev):
        uniforms, uoff, mode = _stream_plan(graph, starts, W, L, rng, uniforms, stream_nodes)
        if biased:
            woff = None
            if uoff is not None:                                 # walk w of start i: uoff[i] + w * L
                woff = (uoff[:, None] + torch.arange(W, dtype=torch.int64, device=dev)[None, :] * L).reshape(-1).contiguous()
            paths = _biased_paths(graph, starts.repeat_interleave(W).contiguous(), L, mode, uniforms, woff, seed, call, W, p, q)
            return paths_topk(paths.view(B, W * L), T)
        ids = torch.empty((B, T), dtype=torch.int32, device=dev)
        counts = torch.empty((B, T), dtype=torch.int32, device=dev)
        nvalid = torch.empty(B, dtype=torch.int32, device=dev)
        packed = use_guide and use_packed
        nv.call("ps_walk_sample", nv.ptr(graph.rowptr), nv.ptr(graph.col), nv.ptr(graph.cdf), graph.V, nv.ptr(starts), B, W, L, T,
                mode | (graph.walk_flags if (use_guide and use_buckets) else 0), nv.ptr(uniforms), nv.ptr(uoff),
                seed & (2 ** 64 - 1), call, nv.ptr(graph.nodeinfo if use_guide else None), nv.ptr(graph.guide if use_guide else None),
                nv.ptr(graph.packed if packed else None),
                nv.ptr(getattr(graph, "buckets", None) if (use_guide and use_buckets) else None),
                nv.ptr(getattr(graph, "dest_info", None) if (packed and use_dest) else None),
                nv.ptr(ids), nv.ptr(counts), nv.ptr(nvalid), nv.stream())
    return NeighborBatch(ids, counts, nvalid)


def _range_tensor(nodes, dev):
    """a python range of node ids as int64 on `dev` (made anew; _range_nodes caches); anything else as it is"""
    return torch.arange(nodes.start, nodes.stop, dtype=torch.int64, device=dev) if isinstance(nodes, range) else nodes


_range_nodes_dev = {}


def _range_nodes(start, stop, dev):
    """arange(start, stop) as int64 on `dev`, made once per (device, start, stop): the item range a model samples is the same on
    every step, and the arange kernel was a launch of its own in each.  Read-only: the kernels take it as const."""
    key = (str(dev), int(start), int(stop))
    t = _range_nodes_dev.get(key)
    if t is None:
        if len(_range_nodes_dev) >= 64:                  # callers that sweep many ranges: do not hold them all
            _range_nodes_dev.clear()
        t = _range_nodes_dev[key] = torch.arange(start, stop, dtype=torch.int64, device=dev)
    return t


def walk_sample_layers(graph, nodes, T, layers, W=100, L=2, rng="numpy", seed=0, call=0, uniforms=None,
                       stream_nodes=None, defer_state=False, p=1.0, q=1.0):
    """`layers` consecutive batch_sample_neighbors calls over the same start nodes (PinSage.get_embeddings,
    model/pinsage.py:271-275) as ONE kernel launch (ps_walk_sample_layers) -> list of NeighborBatch.  Bit-identical
    to `layers` walk_sample calls: Philox uses call, call + 1, ...; rng='numpy' draws all layers' uniforms from the
    global stream in one go (layer 0's, then layer 1's, ... as the reference consumes them) and hands the state back
    once.  `nodes` may be a python range (no host sync in the steady state).  defer_state=True leaves that hand-back to
    dense.finish_rng_state(), which the caller must invoke before it returns to user code.
    p / q other than 1: `layers` consecutive biased walk_sample calls, each drawing from where the previous one left
    np.random (the order of the reference's consecutive calls); the state is handed back before returning, whatever defer_state."""
    dev = graph.device
    if is_biased(p, q) or (rng == "numpy" and graph.has_reachable_sink):
        # a walk that reaches a sink consumes fewer uniforms: the layers are drawn one after the other, each from where the
        # previous one left the stream (what consecutive batch_sample_neighbors calls do in the reference)
        nd = _range_tensor(nodes, dev)
        sn = None if stream_nodes is None else (_range_tensor(stream_nodes[0], dev), stream_nodes[1])
        return [walk_sample(graph, nd, T, W, L, rng=rng, seed=seed, call=call + r, uniforms=None, stream_nodes=sn, p=p, q=q)
                for r in range(layers)]
    as_range = nodes if isinstance(nodes, range) else None
    if as_range is not None:
        if as_range.step != 1 or as_range.start < 0 or as_range.stop > graph.V:
            raise IndexError("list index out of range")
        starts = _range_nodes(as_range.start, as_range.stop, dev)
    else:
        starts = _nodes_tensor(nodes, dev, graph.V)
    B = int(starts.numel())
    ids = torch.empty((layers, B, T), dtype=torch.int32, device=dev)
    counts = torch.empty((layers, B, T), dtype=torch.int32, device=dev)
    nvalid = torch.empty((layers, B), dtype=torch.int32, device=dev)
    stride = 0
    with torch.cuda.device(dev):
        if rng == "numpy":
            # stream offsets: a property of (graph, start nodes, W * L), not of the RNG state.  For a python range of
            # start nodes (what get_embeddings and item shards sample) they are computed once per graph and kept in
            # HBM, like the CSR itself; anything else runs ps_uniform_offsets per call.
            src = stream_nodes[0] if stream_nodes is not None else (as_range if as_range is not None else starts)
            lo = stream_nodes[1] if stream_nodes is not None else 0
            key = ("uoff", src.start, src.stop, W * L) if isinstance(src, range) and src.step == 1 else None
            cache = graph.__dict__.setdefault("_stream_offsets", {})
            if key is not None and key in cache:
                uoff_all, stride = cache[key]
            else:
                all_t = _range_tensor(src, dev) if isinstance(src, range) else _nodes_tensor(src, dev, graph.V)
                uoff_all, total = _uniform_offsets(graph, all_t, W, L)
                stride = int(total.item())
                if key is not None:
                    cache[key] = (uoff_all, stride)
            uoff = uoff_all if stream_nodes is None else uoff_all[lo:lo + B].contiguous()
            mode = nv.PS_RNG_STREAM
            if uniforms is None:
                # an item shard reads only the stream positions of its own start nodes: one run per layer (its bounds are, like
                # the offsets, a property of the graph: fetched once and kept)
                runs = None
                if stream_nodes is not None and B > 0 and B < uoff_all.numel():
                    rkey = None if key is None else key + ("run", lo, B)
                    if rkey is not None and rkey in cache:
                        u_lo, u_hi = cache[rkey]
                    else:
                        u_lo = int(uoff_all[lo].item())
                        u_hi = int(uoff_all[lo + B].item()) if lo + B < uoff_all.numel() else stride
                        if rkey is not None:
                            cache[rkey] = (u_lo, u_hi)
                    if layers <= 3 and os.environ.get("PS_MT_RANGES", "1") != "0":       # PS_MT_RANGES=0: every rank generates the whole stream
                        runs = [(r * stride + u_lo, r * stride + u_hi) for r in range(layers)]
                uniforms, is_raw = draw_numpy_uniforms(layers * stride, dev, defer_state=defer_state, raw=True, ranges=runs)
                mode = nv.PS_RNG_STREAM_RAW if is_raw else nv.PS_RNG_STREAM
        elif rng == "philox":
            uoff, uniforms, mode = None, None, nv.PS_RNG_PHILOX
        else:
            raise ValueError("rng must be 'numpy' or 'philox'")
        # one launch samples up to eight layers of a start node in one wave; deeper models take further launches over the
        # next layers' calls / stream positions (same results: the layers are independent draws)
        for r0 in range(0, layers, 8):
            n = min(8, layers - r0)
            u = uniforms
            if uniforms is not None and r0:
                u = uniforms[2 * r0 * stride:] if mode == nv.PS_RNG_STREAM_RAW else uniforms[r0 * stride:]
            nv.call("ps_walk_sample_layers", nv.ptr(graph.rowptr), nv.ptr(graph.col), nv.ptr(graph.cdf), graph.V, nv.ptr(starts), B,
                    W, L, T, mode | graph.walk_flags, nv.ptr(u), nv.ptr(uoff), stride, seed & (2 ** 64 - 1), call + r0,
                    nv.ptr(graph.nodeinfo), nv.ptr(graph.guide), nv.ptr(graph.packed), nv.ptr(getattr(graph, "buckets", None)),
                    nv.ptr(getattr(graph, "dest_info", None)), n, nv.ptr(ids[r0:r0 + n]), nv.ptr(counts[r0:r0 + n]),
                    nv.ptr(nvalid[r0:r0 + n]), nv.stream())
    return [NeighborBatch(ids[r], counts[r], nvalid[r]) for r in range(layers)]


def walk_paths(graph, starts, L, rng="numpy", seed=0, call=0, walk_mod=0, p=1.0, q=1.0):
    """One walk per start node: int32[B,L] visited nodes (-1 after a sink).  p / q other than 1: ps_walk_paths_biased."""
    dev = graph.device
    biased = is_biased(p, q)
    if biased:
        check_bias(p, q)
        _no_biased_sinks(graph, rng)
    st = _nodes_tensor(starts, dev, graph.V)
    B = int(st.numel())
    paths = torch.empty((B, L), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        uniforms, uoff, mode = _stream_plan(graph, st, 1, L, rng)
        if mode == nv.PS_RNG_STREAM_WALKS:
            mode = nv.PS_RNG_STREAM                              # one walk per start node: a walk's position is its node's
        if biased:
            return _biased_paths(graph, st, L, mode, uniforms, uoff, seed, call, walk_mod, p, q)
        nv.call("ps_walk_paths", nv.ptr(graph.rowptr), nv.ptr(graph.col), nv.ptr(graph.cdf), graph.V, nv.ptr(st), B, L, mode,
                nv.ptr(uniforms), nv.ptr(uoff), seed & (2 ** 64 - 1), call, walk_mod, nv.ptr(graph.nodeinfo), nv.ptr(graph.guide),
                nv.ptr(paths), nv.stream())
    return paths


def importance_pool(x, batch: NeighborBatch = None, ids=None, counts=None, wts=None, nvalid=None, max_idx=None,
                    renorm=True):
    """out[B,H] = sum_j w_j x[ids_j]  (ImportancePooling.forward, model/pinsage.py:101-150)."""
    if batch is not None:
        ids, counts, nvalid = batch.ids, batch.counts, batch.nvalid
    x = x.contiguous()
    if x.dtype != torch.float32:
        raise TypeError("importance_pool expects fp32 features")
    B, T = ids.size(0), ids.size(1)
    N, H = x.size(0), x.size(1)
    out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    if max_idx is None:
        max_idx = N - 1
    with torch.cuda.device(x.device):
        nv.call("ps_importance_pool", nv.ptr(x), N, H, nv.ptr(ids), nv.ptr(counts), nv.ptr(wts), nv.ptr(nvalid), B, T, max_idx,
                int(renorm), nv.ptr(out), nv.stream())
    return out


def _rows_fp32(name, *tensors):
    out = []
    for t in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f"{name} expects fp32 features")
        out.append(t.contiguous())
    return out


def attention_weights(u, v, w2, ids, nvalid):
    """attn[B,T] = softmax over the kept slots j of sum_c w2[c] * relu(u[i,c] + v[ids[i,j],c]), +0.0 elsewhere
    (AttentionAggregator's scores, reference model/aggregators.py:131-151; u / v: the first attention layer split by columns,
    include/pinsage_hip.h)."""
    u, v, w2 = _rows_fp32("attention_weights", u, v, w2.reshape(-1))
    if ids.dtype != torch.int32 or nvalid.dtype != torch.int32:
        raise TypeError("ids / nvalid must be int32")
    B, T = ids.size(0), ids.size(1)
    N, Hd = v.size(0), v.size(1)
    if u.size(0) != B or u.size(1) != Hd or w2.numel() != Hd or nvalid.numel() != B:
        raise ValueError(f"shape mismatch: u {tuple(u.shape)}, v {tuple(v.shape)}, w2 {tuple(w2.shape)}, ids {tuple(ids.shape)}")
    attn = torch.empty((B, T), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        nv.call("ps_attention_weights", nv.ptr(u), nv.ptr(v), N, Hd, nv.ptr(w2), nv.ptr(ids), nv.ptr(nvalid), B, T, nv.ptr(attn),
                nv.stream())
    return attn


def gather_max(x, ids, nvalid):
    """out[B,H] = max over the kept slots j of x[ids[i,j]]; zeros for a row that keeps nothing (MaxPoolingAggregator's
    torch.max over the neighbours, reference model/aggregators.py:195-209)."""
    x, = _rows_fp32("gather_max", x)
    if ids.dtype != torch.int32 or nvalid.dtype != torch.int32:
        raise TypeError("ids / nvalid must be int32")
    B, T = ids.size(0), ids.size(1)
    N, H = x.size(0), x.size(1)
    if nvalid.numel() != B:
        raise ValueError(f"shape mismatch: ids {tuple(ids.shape)}, nvalid {tuple(nvalid.shape)}")
    out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nv.call("ps_gather_max", nv.ptr(x), N, H, nv.ptr(ids), nv.ptr(nvalid), B, T, nv.ptr(out), nv.stream())
    return out


def attention_pool(x, u, v, w2, ids, nvalid):
    """out[B,C] = sum_j attn[i,j] * x[ids[i,j]] with attn = attention_weights(u, v, w2, ids, nvalid): AttentionAggregator.forward
    (reference model/aggregators.py:131-158) as two gathers -- T rows of v, then T rows of x, per output row."""
    attn = attention_weights(u, v, w2, ids, nvalid)
    return importance_pool(x, ids=ids, wts=attn, nvalid=nvalid, renorm=False)


# How the backward of the neighbour gathers runs: "hip" = the transposed gathers of csrc/neigh_agg_bwd.hip (no float atomics: the
# same bits on every run, no [B, T, H] intermediate); "torch" = the torch code that served before (index_add_ for pool, torch
# autograd of the padded [B, T, C] expressions for max and attention), everywhere.
grad_method = "hip"


def _use_hip_grad(*tensors):
    if grad_method not in ("hip", "torch"):
        raise ValueError(f"sampling.grad_method must be 'hip' or 'torch', not {grad_method!r}")
    return grad_method == "hip" and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def slot_lists(ids, nvalid, n_rows, max_idx=None):
    """The transposition of a padded batch: (rptr int64[n_rows + 1], slots int32[B * T]).  slots[rptr[r] : rptr[r + 1]] are the kept
    slots s = i * T + j (j < min(nvalid[i], T), 0 <= ids[i, j] <= min(max_idx, n_rows - 1)) whose id is r, ascending; the entries
    of `slots` from rptr[n_rows] on are the slots that are not kept.  A stable sort plus a search per row: plumbing, built once per
    backward and shared by every transposed gather of it."""
    B, T = int(ids.size(0)), int(ids.size(1))
    if B * T >= 2 ** 31:
        raise ValueError("slot_lists: B * T must stay below 2^31")
    top = n_rows - 1 if max_idx is None else min(int(max_idx), n_rows - 1)
    k = nvalid.clamp(min=0, max=T)
    kept = (torch.arange(T, device=ids.device, dtype=torch.int32)[None, :] < k[:, None]) & (ids >= 0) & (ids <= top)
    key, order = torch.sort(torch.where(kept, ids, n_rows).reshape(-1), stable=True)
    # rptr[r] = the first position whose key is >= r (a search per row: no histogram, nothing waits for the host)
    rptr = torch.searchsorted(key, torch.arange(n_rows + 1, dtype=torch.int32, device=ids.device))
    return rptr, order.to(torch.int32)


def pool_weights(ids, counts=None, wts=None, nvalid=None, max_idx=0, renorm=True, lanes=64):
    """w_eff[B,T]: the weight ps_importance_pool applies to every slot, bit for bit (+0.0 where a slot is not kept); lanes: the
    layout of the forward's weight sum (include/pinsage_hip.h)."""
    B, T = int(ids.size(0)), int(ids.size(1))
    w_eff = torch.empty((B, T), dtype=torch.float32, device=ids.device)
    with torch.cuda.device(ids.device):
        nv.call("ps_pool_weights", nv.ptr(ids), nv.ptr(counts), nv.ptr(wts), nv.ptr(nvalid), B, T, int(max_idx), int(renorm),
                int(lanes), nv.ptr(w_eff), nv.stream())
    return w_eff


def gather_bwd(rptr, slots, n_rows, T, g, coef=None, arg=None):
    """gx[n_rows,H]: the transposed gather of g[B,H] over the slot lists -- weighted by coef[B,T], or restricted to the slots
    arg[B,H] names (ps_gather_bwd)."""
    B, H = int(g.size(0)), int(g.size(1))
    gx = torch.empty((n_rows, H), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        ws, nbytes = nv.workspace("ps_gather_bwd_workspace_bytes", g.device, B, T, H)
        nv.call("ps_gather_bwd", nv.ptr(rptr), nv.ptr(slots), n_rows, T, nv.ptr(coef), nv.ptr(arg), nv.ptr(g), B, H, nv.ptr(gx),
                nv.ptr(ws), nbytes, nv.stream())
    return gx


def gather_max_arg(x, ids, nvalid):
    """(out[B,H], arg int32[B,H]): gather_max and the slot that supplied every maximum (ps_gather_max_arg)"""
    x, = _rows_fp32("gather_max_arg", x)
    if ids.dtype != torch.int32 or nvalid.dtype != torch.int32:
        raise TypeError("ids / nvalid must be int32")
    B, T = ids.size(0), ids.size(1)
    N, H = x.size(0), x.size(1)
    if nvalid.numel() != B:
        raise ValueError(f"shape mismatch: ids {tuple(ids.shape)}, nvalid {tuple(nvalid.shape)}")
    out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    arg = torch.empty((B, H), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        nv.call("ps_gather_max_arg", nv.ptr(x), N, H, nv.ptr(ids), nv.ptr(nvalid), B, T, nv.ptr(out), nv.ptr(arg), nv.stream())
    return out, arg


def attention_bwd_rows(x, u, v, w2, ids, nvalid, attn, g):
    """(ds[B,T], du[B,Hd], dw2[Hd]) of ps_attention_bwd_rows"""
    B, T = int(ids.size(0)), int(ids.size(1))
    N, H, Hd = int(x.size(0)), int(x.size(1)), int(v.size(1))
    ds = torch.empty((B, T), dtype=torch.float32, device=x.device)
    du = torch.empty((B, Hd), dtype=torch.float32, device=x.device)
    dw2 = (torch.empty if B else torch.zeros)(Hd, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws, nbytes = nv.workspace("ps_attention_bwd_rows_workspace_bytes", x.device, B, Hd)
        nv.call("ps_attention_bwd_rows", nv.ptr(x), N, H, nv.ptr(u), nv.ptr(v), Hd, nv.ptr(w2), nv.ptr(ids), nv.ptr(nvalid),
                nv.ptr(attn), nv.ptr(g), B, T, nv.ptr(ds), nv.ptr(du), nv.ptr(dw2), nv.ptr(ws), nbytes, nv.stream())
    return ds, du, dw2


def attention_bwd_cols(rptr, slots, T, ds, u, v, w2):
    """dv[N,Hd] of ps_attention_bwd_cols"""
    B, N, Hd = int(u.size(0)), int(v.size(0)), int(v.size(1))
    dv = torch.empty((N, Hd), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        ws, nbytes = nv.workspace("ps_gather_bwd_workspace_bytes", v.device, B, T, Hd)
        nv.call("ps_attention_bwd_cols", nv.ptr(rptr), nv.ptr(slots), N, T, nv.ptr(ds), nv.ptr(u), nv.ptr(v), Hd, nv.ptr(w2), B,
                nv.ptr(dv), nv.ptr(ws), nbytes, nv.stream())
    return dv


class PoolFn(torch.autograd.Function):
    """Differentiable ps_importance_pool: the forward is the kernel, the backward adds w_ij * grad_out_i into the feature rows
    (d out_i / d x_r = sum over the slots j of row i with ids_ij == r of w_ij).  The weights are the ones the kernel used:
    fp32(count / total) or the given fp32 weights, restricted to the kept slots (j < nvalid, 0 <= id <= max_idx) and, with
    renorm, divided by their fp32 sum (model/pinsage.py:123-146).  grad_method "hip": ps_pool_weights gives those weights bit for
    bit and ps_gather_bwd sums per feature row over the transposed index; "torch": index_add_ of a [B, T, H] product."""

    @staticmethod
    def forward(ctx, x, ids, counts, wts, nvalid, max_idx, renorm):
        x = x.contiguous()
        out = importance_pool(x, ids=ids, counts=counts, wts=wts, nvalid=nvalid, max_idx=max_idx, renorm=renorm)
        ctx.save_for_backward(ids, counts if counts is not None else wts, nvalid)
        ctx.use_counts = counts is not None
        ctx.n_rows = int(x.size(0))
        ctx.max_idx = ctx.n_rows - 1 if max_idx is None else int(max_idx)
        ctx.renorm = bool(renorm)
        # the lane layout of the forward's weight sum (ps_importance_pool's own gate)
        ctx.lanes = 16 if x.size(1) % 4 == 0 and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 else 64
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ids, cw, nvalid = ctx.saved_tensors
        N = ctx.n_rows
        T = ids.size(1)
        # a backward that is itself recorded (create_graph) keeps the differentiable torch code
        if _use_hip_grad(grad_out) and ids.numel() < 2 ** 31 and not (torch.is_grad_enabled() and grad_out.requires_grad):
            g = grad_out.contiguous()                                 # out.sum().backward() hands over a stride-0 tensor
            top = min(ctx.max_idx, N - 1)
            w_eff = pool_weights(ids, cw if ctx.use_counts else None, None if ctx.use_counts else cw, nvalid, top, ctx.renorm,
                                 ctx.lanes)
            rptr, slots = slot_lists(ids, nvalid, N, top)
            return gather_bwd(rptr, slots, N, T, g, coef=w_eff), None, None, None, None, None, None
        slot = torch.arange(T, device=ids.device)[None, :]
        inrow = slot < nvalid[:, None]
        kept = inrow & (ids >= 0) & (ids <= ctx.max_idx)
        if ctx.use_counts:
            tot = (cw * inrow).sum(dim=1, keepdim=True).clamp(min=1)
            w = (cw.double() / tot.double()).float()
        else:
            w = cw
        w = torch.where(kept, w, torch.zeros_like(w))
        if ctx.renorm:
            s = w.sum(dim=1, keepdim=True)
            w = torch.where(s > 0, w / torch.where(s > 0, s, torch.ones_like(s)), w)
        gx = torch.zeros((N, grad_out.size(1)), dtype=grad_out.dtype, device=grad_out.device)
        rows = torch.where(kept, ids, torch.zeros_like(ids)).long()
        gx.index_add_(0, rows.reshape(-1), (grad_out[:, None, :] * w[:, :, None]).reshape(-1, grad_out.size(1)))
        return gx, None, None, None, None, None, None


def pool(x, ids=None, counts=None, wts=None, nvalid=None, max_idx=None, renorm=True):
    """importance_pool that stays on the autograd tape when `x` needs a gradient."""
    if torch.is_grad_enabled() and x.requires_grad:
        return PoolFn.apply(x, ids, counts, wts, nvalid, max_idx, renorm)
    return importance_pool(x, ids=ids, counts=counts, wts=wts, nvalid=nvalid, max_idx=max_idx, renorm=renorm)


def _kept_mask(ids, nvalid, n_rows):
    T = ids.size(1)
    return (torch.arange(T, device=ids.device)[None, :] < nvalid.clamp(min=0, max=T)[:, None]) & (ids >= 0) & (ids < n_rows)


def max_pool_torch(x, ids, nvalid):
    """gather_max as a differentiable torch expression over a padded [B, T, H] tensor (grad_method "torch")"""
    keep = _kept_mask(ids, nvalid, x.size(0))
    t = x[torch.where(keep, ids, torch.zeros_like(ids)).long()]
    t = t.masked_fill(~keep.unsqueeze(2), float("-inf"))
    out = t.max(dim=1).values if ids.size(1) else t.new_zeros((ids.size(0), x.size(1)))
    return torch.where(keep.any(dim=1, keepdim=True), out, torch.zeros_like(out))


def attention_torch(x, u, v, w2, b2, ids, nvalid):
    """attention_pool as a differentiable torch expression over padded [B, T, C] tensors (grad_method "torch")"""
    keep = _kept_mask(ids, nvalid, v.size(0))
    idt = torch.where(keep, ids, torch.zeros_like(ids)).long()
    scores = torch.relu(u[:, None, :] + v[idt]) @ w2.reshape(-1) + b2.reshape(())
    scores = scores.masked_fill(~keep, float("-inf"))
    has = keep.any(dim=1, keepdim=True)
    scores = torch.where(has, scores, torch.zeros_like(scores))
    attn = torch.softmax(scores, dim=1)
    attn = torch.where(keep, attn, torch.zeros_like(attn))
    return (x[idt] * attn.unsqueeze(2)).sum(dim=1)


class MaxPoolFn(torch.autograd.Function):
    """Differentiable ps_gather_max: the forward is ps_gather_max_arg, which also records the slot every maximum came from; the
    backward hands grad_out[i, c] to row ids[i, arg[i, c]] (ps_gather_bwd over the transposed index)."""

    @staticmethod
    def forward(ctx, x, ids, nvalid):
        out, arg = gather_max_arg(x, ids, nvalid)
        ctx.save_for_backward(ids, nvalid, arg)
        ctx.n_rows = int(x.size(0))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        ids, nvalid, arg = ctx.saved_tensors
        g = grad_out.contiguous()
        rptr, slots = slot_lists(ids, nvalid, ctx.n_rows)
        return gather_bwd(rptr, slots, ctx.n_rows, int(ids.size(1)), g, arg=arg), None, None


def max_pool(x, ids, nvalid):
    """gather_max that stays on the autograd tape when `x` needs a gradient."""
    if torch.is_grad_enabled() and x.requires_grad:
        if _use_hip_grad(x) and ids.numel() < 2 ** 31:
            return MaxPoolFn.apply(x, ids, nvalid)
        return max_pool_torch(x, ids, nvalid)
    return gather_max(x, ids, nvalid)


class AttentionFn(torch.autograd.Function):
    """Differentiable attention_pool.  Backward: ps_attention_bwd_rows (ds, du, dw2: one wave per target row), ps_attention_bwd_cols
    (dv) and ps_gather_bwd with coef = attn (dx), the last two over one shared transposition.  The second layer's bias drops out of
    the softmax: its gradient is exactly zero."""

    @staticmethod
    def forward(ctx, x, u, v, w2, b2, ids, nvalid):
        x, u, v, w2 = _rows_fp32("attention", x, u, v, w2.reshape(-1))
        if x.size(0) != v.size(0):
            raise ValueError(f"shape mismatch: x {tuple(x.shape)}, v {tuple(v.shape)}")
        attn = attention_weights(u, v, w2, ids, nvalid)
        out = importance_pool(x, ids=ids, wts=attn, nvalid=nvalid, renorm=False)
        ctx.save_for_backward(x, u, v, w2, ids, nvalid, attn)
        ctx.b2 = (b2.shape, b2.dtype, b2.device)
        ctx.w2_shape = w2.shape
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, u, v, w2, ids, nvalid, attn = ctx.saved_tensors
        need_x, need_u, need_v, need_w2, need_b2 = ctx.needs_input_grad[:5]
        g = grad_out.contiguous()
        N, T = int(x.size(0)), int(ids.size(1))
        dx = du = dv = dw2 = db2 = None
        if need_x or need_v:
            rptr, slots = slot_lists(ids, nvalid, N)
        if need_u or need_v or need_w2:
            ds, du, dw2 = attention_bwd_rows(x, u, v, w2, ids, nvalid, attn, g)
            if need_v:
                dv = attention_bwd_cols(rptr, slots, T, ds, u, v, w2)
        if need_x:
            dx = gather_bwd(rptr, slots, N, T, g, coef=attn)
        if need_b2:
            db2 = torch.zeros(ctx.b2[0], dtype=ctx.b2[1], device=ctx.b2[2])
        return dx, du if need_u else None, dv, dw2 if need_w2 else None, db2, None, None


def attention(x, u, v, w2, b2, ids, nvalid):
    """attention_pool that stays on the autograd tape when one of x, u, v, w2, b2 needs a gradient (b2, the second attention
    layer's bias, receives zeros: it drops out of the softmax)."""
    floats = (x, u, v, w2, b2)
    if torch.is_grad_enabled() and any(t.requires_grad for t in floats):
        if _use_hip_grad(*floats) and ids.numel() < 2 ** 31:
            return AttentionFn.apply(x, u, v, w2, b2, ids, nvalid)
        return attention_torch(x, u, v, w2, b2, ids, nvalid)
    return attention_pool(x, u, v, w2, ids, nvalid)
