"""Hard-negative sampling on the walk kernel.

`NegativeSampler.sample_hard_negatives` of the reference (data/negative_sampler.py:44-99) ranks, per query item,
the nodes visited by 100 `_single_walk` calls by visit count (dict order = first-visit order, stable sort) and
picks negatives from a rank window with `np.random.choice`, everything on the process-global numpy RNG.
Here the 100 walks + ranking of one query are one ps_walk_sample launch (T = 100 * walk_length keeps the whole
ranking); the host-side `np.random.choice` calls are made exactly as in the reference and in the same order, so
with rng='numpy' the returned indices and the final RNG state are identical to the reference's.  A sampler with p or q other
than 1 ranks by its biased walks (the reference ranks with the sampler's own `_single_walk`)."""
from __future__ import annotations

import numpy as np
import torch

from . import sampling

NUM_WALKS = 100            # `for _ in range(100)` at data/negative_sampler.py:67


def sample_hard_negatives(sampler, num_movies, query_indices, num_hard_samples=5, max_rank=5000, min_rank=2000):
    """-> LongTensor [len(query_indices), num_hard_samples] on query_indices.device."""
    if sampler is None:
        raise ValueError("RandomWalkSampler is required for hard negative sampling")
    all_movie_indices = list(range(int(num_movies)))
    L = int(sampler.walk_length)
    hard = []
    for idx in query_indices.cpu().numpy():
        call = sampler._calls
        sampler._calls += 1
        batch = sampling.walk_sample(sampler.graph, [int(idx)], NUM_WALKS * L, W=NUM_WALKS, L=L, rng=sampler.rng,
                                     seed=sampler.seed, call=call, p=getattr(sampler, "p", 1.0), q=getattr(sampler, "q", 1.0))
        ids, _, nvalid, _ = batch.host()
        ranked = ids[0, : int(nvalid[0])]                                   # by count desc, first visit first
        candidates = [int(v) for v in ranked[min_rank:max_rank] if v < num_movies]   # `item in all_movie_indices`
        if not candidates:
            sampled = np.random.choice(all_movie_indices, size=num_hard_samples, replace=False)
        else:
            sampled = np.random.choice(candidates, size=min(num_hard_samples, len(candidates)), replace=False)
            if len(sampled) < num_hard_samples:
                additional = np.random.choice([i for i in all_movie_indices if i not in sampled],
                                              size=num_hard_samples - len(sampled), replace=False)
                sampled = np.concatenate([sampled, additional])
        hard.append(sampled)
    return torch.tensor(np.asarray(hard), device=query_indices.device)


# ---- hard negatives by personalized-PageRank rank (PinSage paper, section 3.3) -----------------------------------------------
# The ranking above holds at most NUM_WALKS * walk_length nodes, so the default window [2000, 5000) of it is always empty and
# every "hard" negative is a uniform random item.  Here the ranking is the query's exact PPR scores over all items
# (pinsage_hip.ppr), the window's members come from one ps_rank_window launch for the whole batch, and the negatives are a
# Floyd subset of them.  The process-global numpy stream is consumed the same way whatever the scores are: 2 B n doubles.

def fill_short_rows(picks, queries, u2, num_movies):
    """picks int[B, n] with -1 in every slot the window could not fill -> int64[B, n], rows distinct and free of the query.
    A -1 slot gets cand = min(floor(u2[b, i] * M), M - 1), M = num_movies, moved on by (cand + 1) % M while cand is the query
    or an earlier slot of the row (slots are filled left to right; the device leaves its -1 slots at the row's end, so the row
    comes out distinct).  Pure host code; needs M > n + 1."""
    out = np.array(picks, dtype=np.int64)
    B, n = out.shape
    M = int(num_movies)
    if M <= n + 1:
        raise ValueError(f"{n} distinct negatives beside the query need more than {n + 1} items, not {M}")
    for b in range(B):
        q = int(queries[b])
        for i in range(n):
            if out[b, i] >= 0:
                continue
            taken = {q} | {int(v) for v in out[b, :i]}
            cand = min(int(np.floor(u2[b, i] * M)), M - 1)
            while cand in taken:
                cand = (cand + 1) % M
            out[b, i] = cand
    return out


def sample_hard_negatives_ppr(sampler, num_movies, query_indices, num_hard_samples=5, max_rank=5000, min_rank=2000):
    """-> LongTensor [len(query_indices), num_hard_samples] on query_indices.device: per query, items ranked
    [min_rank, max_rank) among the items by personalized PageRank from the query (the query itself left out), filled up by
    fill_short_rows where the window is short.  Draws u then u2, [B, n] doubles each, from np.random -- always both."""
    if sampler is None:
        raise ValueError("RandomWalkSampler is required for hard negative sampling")
    queries = query_indices.detach().cpu().numpy().astype(np.int64).reshape(-1)
    B, n, M = int(queries.size), int(num_hard_samples), int(num_movies)
    u = np.random.random_sample((B, n))
    u2 = np.random.random_sample((B, n))
    picks = np.full((B, n), -1, dtype=np.int64)
    if B and n and int(max_rank) > int(min_rank):
        picks = sampler.ppr_rank_window(queries.tolist(), int(min_rank), int(max_rank), n=n, uniforms=u,
                                        max_target=M)[2].cpu().numpy()
    return torch.from_numpy(fill_short_rows(picks, queries, u2, M)).to(query_indices.device)
