"""Item co-occurrence graph of GraphBuilder.build_item_similarity_graph (reference data/graph_builder.py:59-116) on the device.

The reference walks every user's group (groupby('userId'): ascending raw user id, rows in dataframe order) and bumps a dict
entry for every ordered pair of positions; a pair with count >= threshold becomes the two edges [a -> b, b -> a] (a <= b) in
dict insertion order.  Here the counts are one integer GEMM A A^T over the (user, item) multiplicities on the matrix cores
(csrc/cooc_mfma.hip), and the insertion order is rebuilt exactly: a pair enters the dict at (u, p, q) = its first user in
groupby order and the first positions of its items in that user's group (the first two of the item for a self pair), so
sorting the surviving pairs by that key reproduces the reference's edge list, order included.

The pair records have two producers.  "dense" is that GEMM: it needs U x M operand planes, multiplicities <= 127 and counts
inside the operand's exact range.  "sparse" (csrc/cooc_sparse.hip) walks the entry lists row by row with an LDS accumulator:
no planes, no multiplicity limit, counts up to 2^31 - 1, work proportional to the reference's own pair updates.  "auto" runs
dense wherever dense can run and sparse otherwise.  Both are exact, so they return the same tensors.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import native as nv

WINDOW = 512                         # PS_COOC_WINDOW (include/pinsage_hip.h)
_RECORD_BYTES = 16
_FIRST_CAPACITY = 1 << 28            # records (4 GiB) tried first; a larger result reruns the pass once at its exact size
METHODS = ("dense", "sparse", "auto")


def effective_threshold(threshold):
    """The integer t with (count >= threshold) == (count >= t) for every count >= 1 (a pair with count 0 never enters the
    reference's dict); None when no count can pass."""
    t = float(threshold)
    if math.isnan(t) or t > 2.0 ** 62:
        return None
    return 1 if t < 1 else math.ceil(t)


class _Prep:
    """Rows ranked and sorted on the device: user ranks in groupby order, rows grouped by user, distinct entries."""

    def __init__(self, user_ids, item_idx, num_items, dev):
        uid = torch.as_tensor(user_ids).to(dev, torch.int64).reshape(-1)
        it = torch.as_tensor(item_idx).to(dev, torch.int64).reshape(-1)
        if uid.numel() != it.numel():
            raise ValueError("user_ids and item_idx must have the same length")
        M = int(num_items)
        R = it.numel()
        if M <= 0:
            raise ValueError("num_items must be positive")
        if R >= 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 2 rating rows")
        if R and (int(it.min()) < 0 or int(it.max()) >= M):
            raise ValueError("item index out of range [0, num_items)")
        self.M, self.R = M, R
        _, urank = torch.unique(uid, sorted=True, return_inverse=True)       # groupby('userId') order
        self.U = U = int(urank.max()) + 1 if R else 1
        order_u = torch.sort(urank, stable=True).indices                     # (user, row)
        cnt = torch.bincount(urank, minlength=U)
        self.uptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=self.uptr[1:])
        ur = urank[order_u]
        pos = torch.arange(R, device=dev) - self.uptr[ur]
        k1 = ur * M + it[order_u]
        s1 = torch.sort(k1, stable=True)                                     # (user, item, position)
        self.uitem = (s1.values % M).to(torch.int32)
        self.upos = pos[s1.indices].to(torch.int32)
        ekey, mult = torch.unique_consecutive(s1.values, return_counts=True)
        eu, ei = ekey // M, ekey % M
        s2 = torch.sort(ei * U + eu).indices                                 # distinct entries by (item, user)
        self.iuser = eu[s2].to(torch.int32)
        self.iitem = ei[s2].to(torch.int32)
        self.imult = mult[s2].to(torch.int32)
        self.iptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(ei, minlength=M), 0, out=self.iptr[1:])
        self.max_mult = int(mult.max()) if R else 1
        # ordered position pairs (the reference's dict updates): bounds the number of surviving pairs
        d = cnt.to(torch.float64)
        self.updates = int((d * (d - 1) / 2).sum())
        self._by_user = self._max_sq = None

    def by_user(self):
        """(eptr int64[U+1], eitem int32, emult int32): the distinct entries grouped by user, items ascending; built on first
        use (the sparse producer only)."""
        if self._by_user is None:
            s = torch.sort(self.iuser.to(torch.int64) * self.M + self.iitem).indices
            eptr = torch.zeros(self.U + 1, dtype=torch.int64, device=self.iuser.device)
            torch.cumsum(torch.bincount(self.iuser, minlength=self.U), 0, out=eptr[1:])
            self._by_user = (eptr, self.iitem[s].contiguous(), self.imult[s].contiguous())
        return self._by_user

    def max_sq(self):
        """max over items of sum_u m_ua^2: bounds every count (Cauchy-Schwarz)"""
        if self._max_sq is None:
            sq = torch.zeros(self.M, dtype=torch.int64, device=self.iitem.device)
            sq.index_add_(0, self.iitem.to(torch.int64), self.imult.to(torch.int64) ** 2)
            self._max_sq = int(sq.max())
        return self._max_sq

    def row_order(self):
        """int32[M]: item rows by descending work (sum over a row's users of their entry counts), for the sparse producer"""
        eptr = self.by_user()[0]
        work = torch.zeros(self.M, dtype=torch.int64, device=eptr.device)
        work.index_add_(0, self.iitem.to(torch.int64), (eptr[1:] - eptr[:-1])[self.iuser.to(torch.int64)])
        return torch.sort(work, descending=True, stable=True).indices.to(torch.int32)


def _dense_fits(nbytes, device):
    """Whether `auto` may give the dense producer `nbytes` of operand planes: at most half of the free device memory."""
    return nbytes <= torch.cuda.mem_get_info(device)[0] // 2


def _dense_exact_range(max_mult):
    """The count bound (max_sq) below which the dense operand for `max_mult` is exact (ps_cooc_pairs)"""
    return 1 << 24 if max_mult <= 4 else 1 << 31


def _first_capacity(P, capacity, dev):
    if capacity is not None:
        return int(capacity)
    # no pair count is known before the pass: room for every possible pair, up to _FIRST_CAPACITY records and a quarter of
    # the free memory
    return min(P.updates + P.M, P.M * (P.M + 1) // 2, _FIRST_CAPACITY, torch.cuda.mem_get_info(dev)[0] // (4 * _RECORD_BYTES))


def _records_dense(P, thr, capacity, dev, tick):
    """-> (records int32[n, 4]) by the plane contraction (ps_cooc_planes + ps_cooc_pairs)"""
    if P.max_mult > 127:
        raise ValueError(f"a (user, item) pair occurs {P.max_mult} times; the co-occurrence GEMM takes multiplicities up to 127")
    U, M = P.U, P.M
    lib = nv.lib()
    planes, nbytes = nv.workspace("ps_cooc_planes_bytes", dev, U, M, P.max_mult)
    if nbytes == 0:
        raise ValueError(f"co-occurrence shape not supported (users {U}, items {M})")
    stats = torch.empty(3 * M, dtype=torch.int64, device=dev)
    seen = torch.empty(1, dtype=torch.int32, device=dev)
    st = nv.stream()
    nv.call("ps_cooc_planes", nv.ptr(P.iuser), nv.ptr(P.iitem), nv.ptr(P.imult), P.iuser.numel(), U, M, P.max_mult, nv.ptr(planes),
            nbytes, nv.ptr(stats), nv.ptr(seen), st)
    max_sq = int(stats[M:2 * M].max())
    if int(seen) != P.max_mult:
        raise nv.NativeError(f"ps_cooc_planes saw multiplicity {int(seen)}, expected {P.max_mult}")
    tick("planes")
    cap = _first_capacity(P, capacity, dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    h_count = C.c_int64(0)
    for attempt in range(2):
        rec = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
        rc = lib.ps_cooc_pairs(nv.ptr(planes), U, M, P.max_mult, max_sq, nv.ptr(stats), thr, nv.ptr(rec), cap, nv.ptr(count),
                               C.byref(h_count), st)
        if rc == nv.PS_EWORKSPACE and attempt == 0:
            cap = int(h_count.value)
            del rec
            continue
        if rc == nv.PS_EUNSUPPORTED:
            raise ValueError(f"co-occurrence counts may reach {max_sq}: beyond the exact range of the "
                             f"{'fp4' if P.max_mult <= 4 else 'int8'} contraction")
        nv.check(rc, "ps_cooc_pairs")
        break
    n = int(h_count.value)
    del planes
    return rec[:n].clone() if rec.size(0) > n else rec            # frees the first buffer before keys / sort / emit


def _records_sparse(P, thr, capacity, acc_slots, dev):
    """-> (records int32[n, 4]) by the row-wise sparse producer (ps_cooc_pairs_sparse)"""
    U, M = P.U, P.M
    lib = nv.lib()
    slots = int(acc_slots)
    if lib.ps_cooc_pairs_sparse_workspace_bytes(M, slots) == 0:
        raise ValueError(f"sparse co-occurrence: items {M} or acc_slots {slots} not supported")
    max_sq = P.max_sq()
    eptr, eitem, emult = P.by_user()
    order = P.row_order()
    ws, nbytes = nv.workspace("ps_cooc_pairs_sparse_workspace_bytes", dev, M, slots)
    st = nv.stream()
    cap = _first_capacity(P, capacity, dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    h_count = C.c_int64(0)
    for attempt in range(2):
        rec = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
        rc = lib.ps_cooc_pairs_sparse(nv.ptr(P.iptr), nv.ptr(P.iuser), nv.ptr(P.imult), nv.ptr(eptr), nv.ptr(eitem), nv.ptr(emult),
                                      nv.ptr(order), P.iuser.numel(), U, M, max_sq, thr, slots, nv.ptr(rec), cap, nv.ptr(count),
                                      C.byref(h_count), nv.ptr(ws), nbytes, st)
        if rc == nv.PS_EWORKSPACE and attempt == 0:
            cap = int(h_count.value)
            del rec
            continue
        if rc == nv.PS_EUNSUPPORTED:
            raise ValueError(f"co-occurrence counts may reach {max_sq}: beyond the int32 count of a pair record")
        nv.check(rc, "ps_cooc_pairs_sparse")
        break
    n = int(h_count.value)
    return rec[:n].clone() if rec.size(0) > n else rec


def _auto_method(P, dev):
    """dense wherever dense can run, sparse otherwise (no choice by speed)"""
    if P.max_mult > 127 or P.max_sq() >= _dense_exact_range(P.max_mult):
        return "sparse"
    nbytes = nv.lib().ps_cooc_planes_bytes(P.U, P.M, P.max_mult)
    return "dense" if nbytes != 0 and _dense_fits(nbytes, dev) else "sparse"


def item_cooccurrence_graph(user_ids, item_idx, num_items, threshold=5, device="cuda", capacity=None, timer=None, method="dense",
                            acc_slots=0):
    """-> (edge_index int64[2, 2P], edge_weight fp32[2P]) on `device`: the reference's item similarity graph for the rating
    rows (user_ids[r], item_idx[r]) in dataframe order.  user_ids are the raw ids (grouped in ascending order), item_idx the
    mapped item indices in [0, num_items).  `capacity` (records) overrides the first size of the pair buffer; a buffer that
    turns out too small is reallocated once at the exact size and the pass rerun.  `method` picks the producer of the pair
    records: "dense" (a multiplicity above 127, counts beyond the operand's exact range or an unsupported shape raise
    ValueError), "sparse" (counts that may reach 2^31 raise ValueError; `acc_slots` sizes its LDS accumulator, 0 = default) or
    "auto" (dense when dense can run and its planes fit, else sparse).  `timer`, if given, is a callable(name) invoked after
    each phase (for tools/cooc_probe.py)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise nv.NativeError("item_cooccurrence_graph runs on the MI355X; there is no CPU fallback")
    tick = timer or (lambda name: None)
    P = _Prep(user_ids, item_idx, num_items, dev)
    tick("prep")
    thr = effective_threshold(threshold)
    if P.R == 0 or thr is None:
        return torch.empty((2, 0), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.float32, device=dev)
    if method == "auto":
        method = _auto_method(P, dev)
    if method == "dense":
        rec = _records_dense(P, thr, capacity, dev, tick)
    else:
        rec = _records_sparse(P, thr, capacity, acc_slots, dev)
    U, M, R = P.U, P.M, P.R
    n = rec.size(0)
    st = nv.stream()
    tick("pairs")
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    nv.call("ps_cooc_keys", nv.ptr(rec), n, U, M, nv.ptr(P.iptr), nv.ptr(P.iuser), nv.ptr(P.imult), nv.ptr(P.uptr), nv.ptr(P.uitem),
            nv.ptr(P.upos), R, nv.ptr(keys), st)
    tick("keys")
    if n and int(keys.min()) < 0:
        raise nv.NativeError("ps_cooc_keys found no first common user for some pair")
    perm = torch.sort(keys).indices
    del keys
    edge_index = torch.empty((2, 2 * n), dtype=torch.int64, device=dev)
    edge_weight = torch.empty(2 * n, dtype=torch.float32, device=dev)
    nv.call("ps_cooc_emit", nv.ptr(rec), nv.ptr(perm), n, nv.ptr(edge_index), nv.ptr(edge_weight), st)
    tick("order")
    return edge_index, edge_weight
