"""The chunk-local partition of gcn_order_kernel as tests/helpers/gcn_order.py restates it: a permutation, stable inside each
class and chunk, and a tile is flagged exactly when one of its rows keeps a neighbour.  No GPU."""
import numpy as np
import pytest

from helpers import gcn_order as go


@pytest.mark.parametrize("M", go.SIZES + (1, 63, 64, 65, go.CHUNK - 1, go.CHUNK, go.CHUNK + 1))
@pytest.mark.parametrize("name", go.PATTERNS)
def test_partition(M, name):
    keeps = go.pattern(name, M)
    ord_, heavy = go.chunk_partition(keeps)
    ntiles = -(-M // go.TILE)
    assert ord_.shape == (ntiles * go.TILE,) and heavy.shape == (ntiles,) and ord_.dtype == np.int32 and heavy.dtype == np.int32
    assert np.array_equal(np.sort(ord_[:M]), np.arange(M)) and (ord_[M:] == -1).all()
    for r0 in range(0, M, go.CHUNK):
        r1 = min(r0 + go.CHUNK, M)
        o = ord_[r0:r1]
        assert o.min() == r0 and o.max() == r1 - 1                      # a chunk's rows stay in the chunk
        nh = int(keeps[r0:r1].sum())
        assert keeps[o[:nh]].all() and not keeps[o[nh:]].any()          # heavy rows first
        assert (np.diff(o[:nh]) > 0).all() and (np.diff(o[nh:]) > 0).all()      # each class in ascending row order
    padded = np.zeros(ntiles * go.TILE, dtype=bool)
    padded[:M] = keeps[ord_[:M]]
    assert np.array_equal(heavy.astype(bool), padded.reshape(ntiles, go.TILE).any(axis=1))
    tiles = [keeps[ord_[t:min(t + go.TILE, M)]] for t in range(0, M, go.TILE)]
    assert sum(1 for f in tiles if f.any() and not f.all()) <= -(-M // go.CHUNK)     # at most one tile per chunk holds both classes


def test_patterns_plant_what_they_name():
    M = go.SIZES[2]
    nchunks = -(-M // go.CHUNK)
    assert M % go.CHUNK not in (0,) and M % go.TILE != 0 and go.SIZES[0] % go.CHUNK == 0
    assert go.pattern("all", M).all() and not go.pattern("none", M).any()
    for name, row in (("first-of-chunk", go.CHUNK * (nchunks // 2)), ("last-of-chunk", go.CHUNK * (nchunks // 2) - 1), ("last-row", M - 1)):
        assert np.flatnonzero(go.pattern(name, M)).tolist() == [row]
    odd = go.pattern("odd-chunks", M)
    assert [bool(odd[c * go.CHUNK]) for c in range(nchunks)] == [c % 2 == 1 for c in range(nchunks)]
    for name, extra in (("boundary-64j", 0), ("boundary-64j+1", 1)):
        k = go.pattern(name, M)
        counts = [int(k[c * go.CHUNK:(c + 1) * go.CHUNK].sum()) for c in range(nchunks)]
        assert all(n % go.TILE == extra for n in counts[:-1]) and len(set(counts)) > 3
        heavy = go.chunk_partition(k)[1]
        assert [int(heavy[c * go.CHUNK // go.TILE:(c + 1) * go.CHUNK // go.TILE].sum()) for c in range(nchunks - 1)] == \
            [n // go.TILE + extra for n in counts[:-1]]


def test_chunk_size_is_a_parameter_of_the_restatement_only():
    """another chunk size gives another order of the same kind (what a retuned GCN_CHUNK would have to match)"""
    k = go.pattern("random", go.SIZES[1])
    a, b = go.chunk_partition(k, 2048)[0], go.chunk_partition(k, 4096)[0]
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a), np.sort(b))


@pytest.mark.parametrize("M", go.SIZES + (1, 64, 65, go.CHUNK - 1, go.CHUNK, go.CHUNK + 1, 25 * go.CHUNK + 64 * 31 + 5))
def test_blocks_visit_every_tile_once_heavy_tiles_first(M):
    ntiles = -(-M // go.TILE)
    tiles = [go.block_tile(b, ntiles) for b in range(ntiles)]
    assert sorted(tiles) == list(range(ntiles))
    ct = go.CHUNK // go.TILE
    assert [t % ct for t in tiles] == sorted(t % ct for t in tiles)             # round e before round e + 1
    heavy = go.chunk_partition(go.pattern("random", M))[1]
    flags = heavy[tiles]
    if M >= go.MANY_ROWS:                                  # 44 % heavy rows: 14 or 15 heavy tiles of 32 per chunk
        last_heavy = int(np.flatnonzero(flags)[-1])        # before it, light tiles only where a chunk has one heavy tile fewer
        assert last_heavy < 16 * -(-M // go.CHUNK) and (flags[:last_heavy] == 0).sum() <= -(-M // go.CHUNK)
