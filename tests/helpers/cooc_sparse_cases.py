"""Inputs for tests/test_hip_cooc_sparse.py: rating rows (raw user ids, item indices) built so that one mechanism of the sparse
co-occurrence producer (csrc/cooc_sparse.hip) can go wrong at the smallest shape, each with the property it is named for
stated as data the CPU tests check against cooc_defs.pair_table before any device run.

Cases and their restated graphs are cached: a test never mutates what it gets."""
import functools

import numpy as np

import cooc_defs

WINDOW = 512                                     # PS_COOC_WINDOW

# (U, M, R, max multiplicity, threshold): the issue's shapes for "sparse == restatement == dense"
SHAPES = [(1500, 77, 6000, 1, 1), (1500, 77, 6000, 1, 2.5), (1100, 45, 5000, 4, 3), (2100, 130, 9000, 127, 2), (1037, 200, 3000, 3, 1)]
RERUN_SHAPE = (1200, 70, 5000, 2)                # capacity rerun
OVERFLOW_M = 40
OVERFLOW_SLOTS = (1, 3, 8, 0)                    # forced accumulator capacities; 0 = the default


def planted_pairs(U, M):
    """{(a, b): (first common user rank, other common user rank)}: first users at the last / first rank of windows 0, 1, 2 and
    at U - 1 (the last, partial window).  Items M-10 .. M-1 are rated by these users only."""
    return {(M - 10, M - 9): (WINDOW - 1, 1030), (M - 8, M - 7): (WINDOW, 900), (M - 6, M - 5): (2 * WINDOW - 1, U - 1),
            (M - 4, M - 3): (2 * WINDOW, U - 1), (M - 2, M - 1): (U - 1, U - 1)}


@functools.lru_cache(maxsize=None)
def planted(U, M, R, maxm, seed, plant=True):
    """Random rows over U users and items 0 .. M-11 with multiplicities up to maxm (reached exactly), every rank rating at
    least one item, the planted pairs on top, rows shuffled and raw user ids shuffled (rank order == ascending raw id)."""
    rs = np.random.RandomState(seed)
    rank = np.concatenate([np.arange(U), rs.randint(0, U, R)])
    item = rs.randint(0, M - 10, rank.size)
    key = np.unique(rank * M + item)
    rank, item = key // M, key % M
    if maxm > 1:
        k = rs.choice(rank.size, 40, replace=False)
        reps = np.concatenate([[maxm], rs.randint(2, maxm + 1, 39)]) - 1
        rank = np.concatenate([rank, np.repeat(rank[k], reps)])
        item = np.concatenate([item, np.repeat(item[k], reps)])
    if plant:
        rows = [(r, x) for pair, users in planted_pairs(U, M).items() for r in sorted(set(users)) for x in pair]
        rank = np.concatenate([rank, [r for r, _ in rows]])
        item = np.concatenate([item, [x for _, x in rows]])
    perm = rs.permutation(rank.size)
    rank, item = rank[perm], item[perm]
    raw = np.sort(rs.permutation(U) * 7 + 1000)[rank]
    raw.setflags(write=False)
    item.setflags(write=False)
    return raw, item


def shape_case(U, M, R, maxm):
    return planted(U, M, R, maxm, seed=U + M + maxm)


@functools.lru_cache(maxsize=None)
def overflow():
    """M = 40: user 3 rates all 40 items once, 300 more random rows over 700 users (some repeated: self pairs).  Row 0 then has
    39 distinct partners, more than every forced capacity in OVERFLOW_SLOTS."""
    rs = np.random.RandomState(40)
    M = OVERFLOW_M
    users = np.concatenate([np.full(M, 3), rs.randint(0, 700, 300) * 5 + 11])
    items = np.concatenate([np.arange(M), rs.randint(0, M, 300)])
    perm = rs.permutation(users.size)
    users, items = users[perm], items[perm]
    users.setflags(write=False)
    items.setflags(write=False)
    return users, items, M


BIG = 4099                                       # BIG * BIG + 1 = 16 801 802 > 2^24
BIG_ODD = 4097                                   # BIG * BIG_ODD = 16 793 603: odd and > 2^24, not a float32


@functools.lru_cache(maxsize=None)
def beyond_dense():
    """User 50 has BIG rows of item 2, BIG rows of item 5 and BIG_ODD rows of item 7; user 60 has one row of items 2 and 5.
    count(2, 5) = BIG^2 + 1, count(2, 7) = BIG * BIG_ODD (odd, above 2^24: edge_weight rounds it), count(2, 2) =
    BIG (BIG - 1) / 2.  Multiplicity and count bound are both beyond the dense operands."""
    rs = np.random.RandomState(7)
    users = np.concatenate([np.full(2 * BIG + BIG_ODD, 50), [60, 60]])
    items = np.concatenate([np.full(BIG, 2), np.full(BIG, 5), np.full(BIG_ODD, 7), [2, 5]])
    perm = rs.permutation(users.size)
    users, items = users[perm], items[perm]
    users.setflags(write=False)
    items.setflags(write=False)
    return users, items, 9


def multiplicity_128():
    """the arrays of test_hip_cooc.py::test_multiplicity_128_raises"""
    return np.array([5] * 128 + [5, 6, 6]), np.array([3] * 128 + [4, 3, 4]), 10


@functools.lru_cache(maxsize=None)
def restated(case, thr):
    """the restatement's graph of a cached case; case = ("shape", U, M, R, maxm) | ("rerun",) | ("overflow",) | ("beyond",) |
    ("m128",) | ("sampler",)"""
    users, items, M = rows(case)
    ei, ew = cooc_defs.item_similarity_graph(users, items, M, thr)
    ei.setflags(write=False)
    ew.setflags(write=False)
    return ei, ew


def rows(case):
    kind = case[0]
    if kind == "shape":
        U, M, R, maxm = case[1:]
        return (*shape_case(U, M, R, maxm), M)
    if kind == "rerun":
        U, M, R, maxm = RERUN_SHAPE
        return (*planted(U, M, R, maxm, seed=11), M)
    if kind == "overflow":
        return overflow()
    if kind == "beyond":
        return beyond_dense()
    if kind == "m128":
        return multiplicity_128()
    if kind == "sampler":
        return (*planted(1500, 300, 12000, 2, seed=21, plant=False), 300)
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def table(case):
    users, items, M = rows(case)
    return cooc_defs.pair_table(users, items, M)
