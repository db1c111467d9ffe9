"""data.graph_builder -- drop-in for the reference module of the same name (reference data/graph_builder.py).

build_item_similarity_graph is the reference's per-user pair loop (one dict update per ordered pair of positions in every
user's history: ~6.1e9 updates at SYN-25M scale) as an exact integer GEMM on the matrix cores, or, where that GEMM cannot
run (a multiplicity above 127, counts beyond its exact range, planes that do not fit), as an exact row-wise sparse product
(pinsage_hip.cooc, GraphBuilder.cooc_method).  Counts,
threshold, edge order and dtypes are the reference's: pairs in dict insertion order, each as [a -> b, b -> a] with a <= b,
weights = counts as float32; CPU tensors are returned and, as in the reference, self.edge_index / self.edge_weight are NOT
set by it.  build_bipartite_graph and get_adjacency_list are vectorised host versions with the reference's results.
"""
from __future__ import annotations

import numpy as np
import torch

from pinsage_hip import cooc
from pinsage_hip import native as nv


def _lookup(mapping, ids):
    """Vectorised [mapping[x] for x in ids]; the first id missing from the dict raises KeyError, like the dict lookup."""
    ids = np.asarray(ids)
    if ids.size == 0:
        return np.zeros(0, dtype=np.int64)
    keys = np.fromiter(mapping.keys(), dtype=np.result_type(ids.dtype, np.int64), count=len(mapping)) if mapping else np.zeros(0, np.int64)
    vals = np.fromiter(mapping.values(), dtype=np.int64, count=len(mapping)) if mapping else np.zeros(0, np.int64)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    at = np.searchsorted(keys, ids)
    hit = at < keys.size
    hit[hit] = keys[at[hit]] == ids[hit]
    if not hit.all():
        raise KeyError(ids[np.flatnonzero(~hit)[0]].item())
    return vals[at]


class GraphBuilder:
    """
    Builds and manipulates graph structures for recommendation systems.
    """
    cooc_method = "auto"      # producer of the co-occurrence counts: "dense", "sparse" or "auto" (pinsage_hip.cooc)

    def __init__(self, dataset):
        self.dataset = dataset
        self.edge_index = None
        self.edge_weight = None

    def build_bipartite_graph(self):
        """The reference's layout (data/graph_builder.py:21-57): user->movie columns first, user indices offset by the number
        of movies, weights = ratings for both directions; sets self.edge_index / self.edge_weight."""
        print("Building bipartite interaction graph...")
        ratings_df = self.dataset.ratings_df
        u = _lookup(self.dataset.user_id_to_idx, ratings_df['userId'].values)
        m = _lookup(self.dataset.movie_id_to_idx, ratings_df['movieId'].values)
        u = u + len(self.dataset.movie_id_to_idx)
        edge_index = torch.from_numpy(np.stack([np.concatenate([u, m]), np.concatenate([m, u])]).astype(np.int64))
        ratings = ratings_df['rating'].values
        edge_weight = torch.FloatTensor(np.concatenate([ratings, ratings]))
        self.edge_index = edge_index
        self.edge_weight = edge_weight
        print(f"Created bipartite graph with {len(ratings_df)} interactions (bidirectional)")
        return edge_index, edge_weight

    def build_item_similarity_graph(self, threshold=5):
        """Items co-rated by users (data/graph_builder.py:59-116), on the device (pinsage_hip.cooc); CPU tensors out."""
        print("Building item similarity graph...")
        ratings_df = self.dataset.ratings_df
        users = ratings_df['userId'].values
        movies = ratings_df['movieId'].values
        mapping = self.dataset.movie_id_to_idx
        try:
            items = _lookup(mapping, movies)
        except KeyError:
            # the reference raises at the first unmapped movie in groupby order
            order = np.lexsort((np.arange(len(users)), users))
            items = _lookup(mapping, movies[order])
        num_items = max(len(mapping), int(items.max()) + 1 if items.size else 1)
        if items.size and int(items.min()) < 0:
            raise ValueError("movie_id_to_idx holds negative indices")
        dev = nv.require_gpu()
        ei, ew = cooc.item_cooccurrence_graph(torch.from_numpy(np.asarray(users, dtype=np.int64)), torch.from_numpy(items),
                                              num_items, threshold=threshold, device=dev, method=self.cooc_method)
        edge_index, edge_weight = ei.cpu(), ew.cpu()
        print(f"Created item similarity graph with {edge_index.size(1) // 2} unique edges")
        return edge_index, edge_weight

    def get_adjacency_list(self, edge_index, edge_weight=None):
        """adj_list[src] = [(dst, weight), ...] in edge-column order (data/graph_builder.py:118-146)."""
        max_node_idx = edge_index.max().item() + 1
        src = edge_index[0].cpu().numpy().astype(np.int64)
        dst = edge_index[1].tolist()
        w = edge_weight.tolist() if edge_weight is not None else [1.0] * len(dst)
        if src.size and (src.min() < -max_node_idx):
            raise IndexError("list index out of range")
        src = np.where(src < 0, src + max_node_idx, src)          # a python list index wraps
        order = np.argsort(src, kind="stable")
        bounds = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=max_node_idx))]).tolist()
        pairs = [(dst[k], w[k]) for k in order.tolist()]
        return [pairs[bounds[i]:bounds[i + 1]] for i in range(max_node_idx)]
