"""The restatement and the case table of the second level of the two-level search (csrc/rerank.hip: ps_rerank_topk), shared by
tests/test_rerank_cases.py (CPU: the table contains what its cases are named for, and the restatement agrees with a brute-force
statement), tests/test_hip_rerank.py (GPU: every case bit for bit) and tests/helpers/abi_cases_rerank.py (the contract case).
numpy only.

  restate      similarities from the C oracle's k-ordered fmaf chain (oracle.c_oracle.linear, indexed per pair, as
               gemm_cases.ref_prenorm takes them), keys from topk_cases.make_keys("dot", ...): the distinct valid ids of a row,
               sorted by key, the first k, padded with (-inf, -1).
  the table    cases(): name -> Case, the smallest shapes that reach every branch of the kernel (64 candidates per lane round,
               32 columns per tile, 16-byte and 4-byte loads, the limit-sized list).
  the fixture  recall_fixture(): clustered unit vectors on which re-ranking must raise the recall of the Hamming order.
"""
import functools
from collections import namedtuple

import numpy as np

from helpers import topk_cases as tk

LANES = 64                # candidates of one lane round                      (c0 += 64)
TILE_COLS = 32            # columns staged per tile                           (constexpr int RR_DC = 32)
MIN_LIMIT = 4096          # ps_rerank_max_candidates() returns at least this

# offset: E and Q are handed to the kernel as views that many floats into a larger buffer (0: as allocated)
Case = namedtuple("Case", "name E Q cand k id_offset offset")


def similarities(E, Q):
    """fp32 [nq, N]: Q_i . E_j by the C oracle's chain (columns ascending, one fmaf each, from +0.0)"""
    from oracle import c_oracle as co
    return co.linear(np.ascontiguousarray(Q, dtype=np.float32), np.ascontiguousarray(E, dtype=np.float32), threads=8)


def valid_rows(cand_row, N, id_offset):
    """the distinct rows of E a candidate list names, ascending (python ints: an offset of 2^33 and ids near the int64 ends)"""
    return sorted({int(c) - int(id_offset) for c in cand_row if 0 <= int(c) - int(id_offset) < N})


def restate(E, Q, cand, k, id_offset=0, sims=None):
    """-> (vals fp32 [nq, k], ids int64 [nq, k]) as ps_rerank_topk defines them"""
    E, Q, cand = np.asarray(E, dtype=np.float32), np.asarray(Q, dtype=np.float32), np.asarray(cand, dtype=np.int64)
    N, nq = E.shape[0], Q.shape[0]
    assert cand.shape[0] == nq and Q.shape[1] == E.shape[1]
    sims = similarities(E, Q) if sims is None else sims
    vals = np.full((nq, k), -np.inf, dtype=np.float32)
    ids = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        rows = np.array(valid_rows(cand[i], N, id_offset), dtype=np.int64)
        if not len(rows):
            continue
        s = sims[i, rows]
        o = np.argsort(tk.make_keys("dot", s, rows), kind="stable")[:k]
        vals[i, :len(o)], ids[i, :len(o)] = s[o], rows[o] + int(id_offset)
    return vals, ids


def same(a, b):
    return tk.same(a, b)


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _gauss(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


def _perm_lists(rs, N, nq, R):
    return np.stack([rs.permutation(N)[:R] for _ in range(nq)]).astype(np.int64)


def _plain(name, seed, D, N, nq, R, k, id_offset=0, offset=0):
    rs = np.random.RandomState(seed)
    return Case(name, _gauss(rs, N, D), _gauss(rs, nq, D), _perm_lists(rs, N, nq, R) + id_offset, k, id_offset, offset)


def _invalid():
    """pads inside the lists, ids >= N, negative ids; row 1 has fewer than k valid candidates, row 2 one, row 3 none"""
    rs = np.random.RandomState(31)
    N, D, nq, R, k = 50, 8, 4, 20, 6
    cand = _perm_lists(rs, N, nq, R)
    cand[0, [2, 9, 19]] = (-1, N, -7)
    cand[1, :] = -1
    cand[1, [0, 5, 11, 18]] = (7, N + 3, 21, 3)
    cand[2, :] = (-1, N, 2 ** 40, -2 ** 40, -2 ** 63, 2 ** 63 - 1, N + 1, -2, -1, -1, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1)
    cand[3, :] = [-1, N, -3, 2 ** 31, 2 ** 32, -1, -1, N, N, -1] * 2
    return Case("invalid-ids", _gauss(rs, N, D), _gauss(rs, nq, D), cand, k, 0, 0)


def _duplicates():
    """every id twice -- side by side, a lane round apart in spirit (first and second half), and interleaved; k above the 8 distinct"""
    rs = np.random.RandomState(32)
    N, D, nq, k = 40, 8, 3, 10
    a = _perm_lists(rs, N, nq, 8)
    cand = np.stack([np.repeat(a[0], 2), np.concatenate([a[1], a[1]]), np.concatenate([a[2], a[2][::-1]])])
    return Case("duplicates", _gauss(rs, N, D), _gauss(rs, nq, D), cand, k, 0, 0)


TINY = np.float32(1e-30)          # normal; TINY * TINY underflows to a zero of the product's sign


def _ties_zeros():
    """rows 0-3 and 4-7 of E identical under different ids (ties by ascending id); rows 8 / 9 give query 0 the similarity +0.0
    (positive products that underflow; a zero row); with rows 10 / 11 every product is negative and underflows, so the bare
    chain ends in -0.0 (from +0.0 it gets there in no other way) -- the exact search reports that pair as +0.0, because its
    GEMM adds the absent bias as +0.0 (oracle/pinsage_oracle.c orc_linear does the same), and so does the re-rank: the four
    rows tie and come out by id"""
    rs = np.random.RandomState(33)
    N, D = 24, 4
    E = _gauss(rs, N, D)
    E[1:4] = E[0]
    E[5:8] = E[4]
    E[8], E[9], E[10], E[11] = TINY, 0.0, -TINY, -TINY
    Q = _gauss(rs, 2, D)
    Q[0] = TINY
    cand = np.stack([rs.permutation(N)[:20], rs.permutation(N)[:20]]).astype(np.int64)
    cand[0, :12] = rs.permutation(12)            # all twelve planted rows in query 0's list, in some order
    cand[0, 12:] = 12 + rs.permutation(12)[:8]
    return Case("ties-zeros", E, Q, cand, 20, 0, 0)


def _big_offset():
    off = 2 ** 33
    c = _plain("offset-2^33", 34, 8, 60, 3, 20, 5, id_offset=off)
    cand = c.cand.copy()
    cand[0, :4] = (3, off - 1, off + 60, -1)     # a row index without the offset, and the ids either side of the table
    return c._replace(cand=cand)


def limit():
    """the library's ps_rerank_max_candidates()"""
    from helpers import abi_cases as ac
    return int(ac.lib().ps_rerank_max_candidates())


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case"""
    out = [
        _plain("smallest", 1, 1, 5, 1, 1, 1),
        _plain("d3-scalar-all-emitted", 2, 3, 70, 3, 63, 63),
        _plain("d4-r64-k1", 3, 4, 90, 3, 64, 1),
        _plain("d4-r65-k33", 4, 4, 90, 3, 65, 33),
        _plain("d130-unaligned", 5, 130, 100, 5, 40, 7, offset=1),
        _plain("d132-unaligned", 6, 132, 100, 5, 40, 7, offset=1),       # 16-byte shape, 4-byte pointers
        _plain("d256-main", 7, 256, 1000, 65, 110, 11),
        _plain("limit-R", 8, 8, 5000, 2, limit(), 100),
        _invalid(),
        _duplicates(),
        _ties_zeros(),
        _big_offset(),
    ]
    d = {c.name: c for c in out}
    assert len(d) == len(out)
    for c in out:
        for a in (c.E, c.Q, c.cand):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(name):
    """restate of a table case, computed once, read-only"""
    c = cases()[name]
    v, i = restate(c.E, c.Q, c.cand, c.k, c.id_offset)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


# ---- the recall fixture ----------------------------------------------------------------------------------------------------------
RECALL_SETTINGS = ((5, 4), (5, 10), (10, 10))          # (k, factor): R = 20 (MFMA scan), 50 (popcount scan), 100 (large-k form)
RECALL_BITS = 256


@functools.lru_cache(maxsize=None)
def recall_fixture():
    """(x fp32 [4200, 64] unit rows around 40 Gaussian centres, queries = its first 64 rows)"""
    rs = np.random.RandomState(4242)
    centres = rs.standard_normal((40, 64))
    x = centres[rs.randint(0, 40, size=4200)] + 0.7 * rs.standard_normal((4200, 64))
    x = (x / np.sqrt((x * x).sum(axis=1))[:, None]).astype(np.float32)
    x.setflags(write=False)
    return x, x[:64]


@functools.lru_cache(maxsize=None)
def recall_truth(k):
    """int64 [64, k]: the exact search's ids for the fixture's queries (the restatement over every item)"""
    x, q = recall_fixture()
    ids = restate(x, q, np.tile(np.arange(len(x)), (len(q), 1)), k, sims=recall_sims())[1]
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def recall_sims():
    x, q = recall_fixture()
    s = similarities(x, q)
    s.setflags(write=False)
    return s


def hits(found, truth):
    """int [nq]: per query, how many of truth's ids the row of `found` holds"""
    return np.array([np.intersect1d(f[f >= 0], t).size for f, t in zip(np.asarray(found), np.asarray(truth))])
