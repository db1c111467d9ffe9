"""data.negative_sampler -- drop-in for the reference module of the same name (reference data/negative_sampler.py): the
NegativeSampler class run.py builds, with the reference's constructor, attributes and method signatures.

Random negatives are ONE `np.random.choice(all_movie_indices, size=num_negative_samples, replace=False)` call on the process-
global numpy stream, exactly the reference's, so the indices and the stream's state afterwards are the reference's.  Hard
negatives run the 100 walks and the visit-count ranking of a query on the device (pinsage_hip.negatives, one ps_walk_sample
launch per query) and make the reference's `np.random.choice` calls on the host in the reference's order.
"""
from __future__ import annotations

import numpy as np
import torch

from pinsage_hip import negatives


class NegativeSampler:
    # which ranking the hard negatives' [min_rank, max_rank) window is cut from.  "walk" (default): the reference's, the nodes
    # seen by 100 walks -- at most 100 * walk_length of them, so the default window [2000, 5000) is empty and every negative is a
    # random item.  "ppr": the query's personalized-PageRank ranking over all items, the PinSage paper's hard negatives
    # (pinsage_hip.negatives.sample_hard_negatives_ppr); it consumes the numpy stream differently from the reference.
    hard_method = "walk"

    def __init__(self, dataset, random_walk_sampler=None, num_negative_samples=500):
        self.dataset = dataset
        self.random_walk_sampler = random_walk_sampler
        self.num_negative_samples = num_negative_samples
        self.all_movie_indices = list(range(len(dataset.movie_id_to_idx)))

    def sample_random_negatives(self, batch_size, device):
        """LongTensor [num_negative_samples] on `device`: distinct item indices, shared by the whole batch"""
        picked = np.random.choice(self.all_movie_indices, size=self.num_negative_samples, replace=False)
        return torch.tensor(picked, device=device)

    def sample_hard_negatives(self, query_indices, num_hard_samples=5, max_rank=5000, min_rank=2000):
        """LongTensor [len(query_indices), num_hard_samples] on query_indices.device: items from the [min_rank, max_rank) window
        of each query's visit-count ranking, filled up with random items where the window is short"""
        if self.hard_method not in ("walk", "ppr"):
            raise ValueError(f"hard_method must be 'walk' or 'ppr', not {self.hard_method!r}")
        fn = negatives.sample_hard_negatives if self.hard_method == "walk" else negatives.sample_hard_negatives_ppr
        return fn(self.random_walk_sampler, len(self.all_movie_indices), query_indices,
                  num_hard_samples=num_hard_samples, max_rank=max_rank, min_rank=min_rank)

    def sample_batch_negatives(self, query_indices, device, epoch=0):
        """(random negatives, hard negatives or None): hard negatives from epoch 1 on when a walk sampler was given, min(epoch, 6)
        per query"""
        random_negatives = self.sample_random_negatives(len(query_indices), device)
        if epoch >= 1 and self.random_walk_sampler is not None:
            return random_negatives, self.sample_hard_negatives(query_indices, num_hard_samples=min(epoch, 6))
        return random_negatives, None
