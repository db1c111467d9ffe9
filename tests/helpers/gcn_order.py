"""The chunk-local row order of the fused GCN layer (csrc/dense_mfma.hip: gcn_order_kernel, ps_gcn_order), restated in numpy, and
the class patterns its tests plant.  No GPU, no library."""
import numpy as np

CHUNK = 2048                              # rows per workgroup of gcn_order_kernel (GCN_CHUNK)
TILE = 64                                 # rows of a GEMM tile; ord[64 t .. 64 t + 63] is tile t
MANY_ROWS = 64 * 384                      # ps_gcn_layer serves M >= 24 576
SIZES = (MANY_ROWS, MANY_ROWS + 1, MANY_ROWS + 4096 + 63)      # whole tiles; a clamped last tile; a partial last chunk


def _cdiv(a, b):
    return -(-a // b)


def chunk_partition(keeps, chunk=CHUNK):
    """(ord int32[64 ceil(M / 64)], tile_heavy int32[ceil(M / 64)]) of bool[M] `keeps`: per chunk of `chunk` consecutive rows the
    rows that keep a neighbour ascending, then the others ascending; -1 from M on.  Tile t of a chunk with nh such rows is
    flagged when 64 t < nh -- the kernel's arithmetic; that this is "any row of the tile keeps" is what the CPU test asserts."""
    assert chunk % TILE == 0
    M = keeps.size
    ntiles = _cdiv(M, TILE)
    ord_ = np.full(ntiles * TILE, -1, dtype=np.int32)
    heavy = np.zeros(ntiles, dtype=np.int32)
    for r0 in range(0, M, chunk):
        r1 = min(r0 + chunk, M)
        f = keeps[r0:r1]
        i = np.arange(r0, r1, dtype=np.int32)
        nh = int(f.sum())
        ord_[r0:r0 + nh] = i[f]
        ord_[r0 + nh:r1] = i[~f]
        t = np.arange(_cdiv(r1 - r0, TILE))
        heavy[r0 // TILE + t] = TILE * t < nh
    return ord_, heavy


PATTERNS = ("all", "none", "first-of-chunk", "last-of-chunk", "last-row", "odd-chunks", "boundary-64j", "boundary-64j+1", "random")


def pattern(name, M, chunk=CHUNK):
    """bool[M]: which rows keep a neighbour"""
    k = np.zeros(M, dtype=bool)
    nchunks = _cdiv(M, chunk)
    if name == "all":
        k[:] = True
    elif name == "none":
        pass
    elif name == "first-of-chunk":                        # exactly one heavy row: the first row of a chunk
        k[chunk * (nchunks // 2)] = True
    elif name == "last-of-chunk":                         # ... the last row of a chunk
        k[chunk * (nchunks // 2) - 1] = True
    elif name == "last-row":                              # ... row M - 1
        k[M - 1] = True
    elif name == "odd-chunks":
        for c in range(1, nchunks, 2):
            k[c * chunk:(c + 1) * chunk] = True
    elif name in ("boundary-64j", "boundary-64j+1"):      # chunk c holds 64 (c + 1) (+ 1) heavy rows, scattered over the chunk
        rs = np.random.RandomState(64)
        for c in range(nchunks):
            rows = min(chunk, M - c * chunk)
            nh = min(TILE * (c % 7 + 1) + (name == "boundary-64j+1"), rows)
            k[c * chunk + rs.choice(rows, nh, replace=False)] = True
    elif name == "random":
        k[:] = np.random.RandomState(7).random_sample(M) < 0.44
    else:
        raise KeyError(name)
    return k


def block_tile(b, ntiles, chunk=CHUNK):
    """the tile block b of the layer GEMM runs (gcn_block_tile): round by round -- tile 0 of every chunk, tile 1 of every chunk,
    ... -- so that the heavy tiles, the first ones of every chunk, are the first blocks of the launch"""
    ct = chunk // TILE
    nfull, tail = divmod(ntiles, ct)
    head = tail * (nfull + 1)
    if b < head:
        return (b % (nfull + 1)) * ct + b // (nfull + 1)
    b -= head
    return (b % nfull) * ct + tail + b // nfull
