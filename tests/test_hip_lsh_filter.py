"""The staged LSH encode (csrc/lsh_filter.hip: ps_lsh_stage + ps_lsh_encode with PS_LSH_STAGED -- signs from a split-bf16 MFMA
estimate where it is beyond doubt, the exact fmaf chain elsewhere) against the C oracle, bit for bit.  Both row tiles (64 and
128 rows per workgroup: the launcher picks by size, PS_LSH_ROWS forces one) run every data case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

from oracle import c_oracle as co
from oracle import pinsage_oracle as orc

TILES = (64, 128)
SHAPES = ((32, 32), (64, 96), (128, 256), (256, 512))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _encode(x, A, monkeypatch, tile, stats=False):
    """(codes as numpy, the StagedLsh) of dense.lsh_encode over dense.stage_lsh(A)"""
    from pinsage_hip import dense
    monkeypatch.setenv("PS_LSH_ROWS", str(tile))
    if stats:
        monkeypatch.setenv("PS_LSH_STATS", "1")
    else:
        monkeypatch.delenv("PS_LSH_STATS", raising=False)
    S = dense.stage_lsh(_dev(A))
    assert isinstance(S, dense.StagedLsh)
    return dense.lsh_encode(_dev(x), S).cpu().numpy(), S


def _check(x, A, monkeypatch, what, tiles=TILES):
    want = co.lsh_encode(x, A, threads=8)
    for tile in tiles:
        got, _ = _encode(x, A, monkeypatch, tile)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}, {tile}-row tile: {len(bad)} code bytes differ, first at (row, byte) {bad[0]}"
    return want


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("D,nbits", SHAPES)
def test_ragged_tiles(D, nbits, tile, monkeypatch):
    rs = np.random.RandomState(D + tile)
    x = rs.standard_normal((2 * tile + 3, D)).astype(np.float32)
    A = rs.standard_normal((nbits, D)).astype(np.float32)
    want = co.lsh_encode(x, A, threads=8)
    for n in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
        got, _ = _encode(x[:n], A, monkeypatch, tile)
        assert np.array_equal(got, want[:n]), n


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -40, 2.0 ** 40])
def test_exact_zeros_in_bulk(scale, monkeypatch):
    """+-1 entries at D = 32: one dot in seven is exactly 0 and encodes as 1; scaled rows leave the norm range of the filter"""
    rs = np.random.RandomState(7)
    x = rs.choice([-1.0, 1.0], size=(300, 32)).astype(np.float32)
    A = rs.choice([-1.0, 1.0], size=(64, 32)).astype(np.float32)
    zero = (x.astype(np.float64) @ A.astype(np.float64).T) == 0
    assert 0.12 < zero.mean() < 0.16
    want = _check(x * np.float32(scale), A, monkeypatch, f"scale {scale}")
    bits = np.unpackbits(want, axis=1, bitorder="little").astype(bool)
    assert bits[zero].all()


def test_planted_rows(monkeypatch):
    rs = np.random.RandomState(11)
    x = rs.standard_normal((70, 64)).astype(np.float32)
    A = rs.standard_normal((96, 64)).astype(np.float32)
    x[0] = 0.0
    x[1] = 0.0
    x[1, 0], x[1, 1] = 1.0, -1.0
    A[3] = 0.0
    A[3, 0] = A[3, 1] = 1.0
    A[4] = -A[3]
    A[5] = 0.0
    want = _check(x, A, monkeypatch, "plants")
    bits = np.unpackbits(want, axis=1, bitorder="little")
    assert bits[0].all() and bits[1, 3] == 1 and bits[1, 4] == 1 and bits[:, 5].all()


@pytest.mark.parametrize("tile", TILES)
def test_everything_flagged(tile, monkeypatch):
    """more flagged dots than one round of the recheck list takes: x all zero, then A all zero"""
    rs = np.random.RandomState(13)
    n, D, nbits = 2 * tile + 3, 256, 512
    A = rs.standard_normal((nbits, D)).astype(np.float32)
    got, S = _encode(np.zeros((n, D), dtype=np.float32), A, monkeypatch, tile, stats=True)
    assert (got == 0xFF).all()
    torch.cuda.synchronize()
    assert S.stats() == (n * nbits, n * nbits)
    x = rs.standard_normal((n, D)).astype(np.float32)
    got, S = _encode(x, np.zeros((nbits, D), dtype=np.float32), monkeypatch, tile, stats=True)
    assert (got == 0xFF).all() and S.stats() == (n * nbits, n * nbits)


def _fma32(a, b, c):
    return orc._fmaf_vec(np.float32(a).reshape(1), np.float32(b).reshape(1), np.float32(c).reshape(1))[0]


def test_hairs_breadth(monkeypatch):
    """64 (row, bit) pairs whose exact chain ends a rounding error away from zero, 32 on either side: the last coordinate of
    the row is chosen, with the oracle's own fma, so that it nearly cancels the chain over the coordinates before it"""
    D, nbits = 256, 512
    A = orc.lsh_rotation_matrix(D, nbits)
    rs = np.random.RandomState(17)
    x = rs.standard_normal((64, D)).astype(np.float32)
    x[:, -1] = 0.0
    _, part = orc.lsh_encode(x, A)                                 # fma(0, a, p) = p: the chain before the last coordinate
    js = rs.permutation(nbits)[:64]
    sides = []
    for i, j in enumerate(js):
        p, a = part[i, j], A[j, -1]
        t = np.float32(-p / a)
        cand = [t]
        for _ in range(4):
            cand = [np.nextafter(cand[0], np.float32(-np.inf))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
        ends = [(float(_fma32(c, a, p)), c) for c in cand]
        want_neg = i % 2 == 1
        pick = [(abs(e), c) for e, c in ends if (e < 0) == want_neg]
        assert pick, (i, j)
        e, c = min(pick, key=lambda q: q[0])
        assert e <= 8 * np.spacing(np.float32(abs(p)))             # a few ulp of the partial chain
        x[i, -1] = c
        sides.append(want_neg)
    want = _check(x, A, monkeypatch, "hair's breadth")
    bits = np.unpackbits(want, axis=1, bitorder="little")
    assert [bits[i, j] == 0 for i, j in enumerate(js)] == sides


def test_non_finite(monkeypatch):
    rs = np.random.RandomState(19)
    D, nbits = 128, 256
    x = rs.standard_normal((140, D)).astype(np.float32)
    A = rs.standard_normal((nbits, D)).astype(np.float32)
    x[2, 5] = np.nan
    x[3, 7] = np.inf
    x[4, 1], x[4, 100] = np.inf, -np.inf
    A[9, 3] = np.inf
    A[200, 64] = -np.inf
    want = _check(x, A, monkeypatch, "nan / inf")
    bits = np.unpackbits(want, axis=1, bitorder="little")
    assert not bits[2].any()                                       # a NaN chain is not >= 0
    nan4 = np.sign(A[:, 1]) == np.sign(A[:, 100])                  # inf a - inf a': NaN where the two products differ in sign
    nan4[[9, 200]] = False
    assert nan4.sum() > 64 and not bits[4][nan4].any()
    big_x = (rs.standard_normal((70, D)) * 1e30).astype(np.float32)
    big_A = (rs.standard_normal((nbits, D)) * 1e30).astype(np.float32)
    _check(big_x, big_A, monkeypatch, "overflowing chain")
    _check(big_x, A, monkeypatch, "huge rows")


@pytest.fixture(scope="module")
def unit_rows():
    out = {}
    for D, nbits in ((256, 512), (128, 256)):
        rs = np.random.RandomState(D)
        x = rs.standard_normal((2000, D)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
        A = orc.lsh_rotation_matrix(D, nbits)
        out[D] = (x, A, co.lsh_encode(x, A, threads=8))
    return out


@pytest.mark.parametrize("D", [256, 128])
def test_same_answer_three_ways(D, unit_rows, monkeypatch):
    from pinsage_hip import dense
    from pinsage_hip import native as nv
    x, A, want = unit_rows[D]
    xd, Ad = _dev(x), _dev(A)
    monkeypatch.delenv("PS_LSH_ROWS", raising=False)
    monkeypatch.delenv("PS_LSH_STATS", raising=False)
    S = dense.stage_lsh(Ad)
    W = dense.stage_weight(Ad)
    assert isinstance(S, dense.StagedLsh) and isinstance(W, dense.StagedWeight)
    out = []
    for ptr, flags in ((S.image, nv.PS_LSH_STAGED), (Ad, 0), (W.t, nv.PS_WPERM)):
        codes = torch.empty((x.shape[0], A.shape[0] // 8), dtype=torch.uint8, device="cuda")
        nv.call("ps_lsh_encode", nv.ptr(xd), x.shape[0], D, nv.ptr(ptr), A.shape[0], nv.ptr(codes), flags, nv.stream())
        out.append(codes.cpu().numpy())
    assert np.array_equal(out[0], want) and np.array_equal(out[1], want) and np.array_equal(out[2], want)
    monkeypatch.setenv("PS_LSH_FILTER", "0")                       # the switch back to the fp32 kernels
    assert isinstance(dense.stage_lsh(Ad), dense.StagedWeight)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("D", [256, 128])
def test_the_filter_filters(D, tile, unit_rows, monkeypatch):
    """the share of dots that take the exact chain: erf(c sqrt(D / 2)) = 0.30 % / 0.21 % expected on unit-norm rows against an
    orthonormal frame, capped at 1 %; never zero.  (A kernel that rechecked every dot would pass every other test here.)"""
    x, A, want = unit_rows[D]
    got, S = _encode(x, A, monkeypatch, tile, stats=True)
    assert np.array_equal(got, want)
    seen, flagged = S.stats()
    print(f"D = {D}, {tile}-row tile: {flagged} of {seen} dots flagged = {100.0 * flagged / seen:.3f} %")
    assert seen == x.shape[0] * A.shape[0]
    assert 0 < flagged <= 0.01 * seen
    got, _ = _encode(x, A, monkeypatch, tile, stats=False)         # switched off: the counters stay
    assert np.array_equal(got, want) and S.stats() == (seen, flagged)


def test_restaging_follows_the_matrix(monkeypatch):
    from pinsage_hip import dense
    from pinsage_hip.shard import ShardedPinSage
    monkeypatch.delenv("PS_LSH_ROWS", raising=False)
    rs = np.random.RandomState(23)
    x = rs.standard_normal((500, 256)).astype(np.float32)
    A = orc.lsh_rotation_matrix(256, 512)
    Ad, xd = _dev(A), _dev(x)
    pipe = ShardedPinSage({}, 2, None, 500)
    c1 = pipe.build_index(xd, Ad).cpu().numpy()
    assert isinstance(pipe._staged["A"][2], dense.StagedLsh)
    assert np.array_equal(c1, co.lsh_encode(x, A, threads=8))
    first = pipe._staged["A"][2]
    assert pipe._staged_A(Ad) is first                             # staged once per matrix
    Ad.neg_()
    c2 = pipe.build_index(xd, Ad).cpu().numpy()
    assert pipe._staged["A"][2] is not first
    assert np.array_equal(c2, co.lsh_encode(x, -A, threads=8)) and not np.array_equal(c1, c2)


def test_abi_errors():
    from pinsage_hip import native as nv
    L = nv.lib()
    assert L.ps_lsh_stage_bytes(512, 256) > 512 * 256 * 8 and L.ps_lsh_stage_bytes(32, 32) > 0
    for nbits, D in ((512, 48), (40, 32), (2048, 256), (512, 512), (0, 32), (32, 0)):
        assert L.ps_lsh_stage_bytes(nbits, D) == 0, (nbits, D)
    A = torch.randn(64, 32, device="cuda")
    nb = L.ps_lsh_stage_bytes(64, 32)
    img = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    st = nv.stream()
    assert L.ps_lsh_stage(nv.ptr(A), 64, 32, nv.ptr(img), nb, st) == nv.PS_OK
    assert L.ps_lsh_stage(nv.ptr(A), 64, 32, nv.ptr(img), nb - 1, st) == nv.PS_EINVAL          # short buffer
    assert L.ps_lsh_stage(None, 64, 32, nv.ptr(img), nb, st) == nv.PS_EINVAL
    assert L.ps_lsh_stage(nv.ptr(A), 64, 32, None, nb, st) == nv.PS_EINVAL
    assert L.ps_lsh_stage(nv.ptr(A), 40, 32, nv.ptr(img), nb, st) == nv.PS_EUNSUPPORTED        # unserved shapes
    assert L.ps_lsh_stage(nv.ptr(A), 64, 48, nv.ptr(img), nb, st) == nv.PS_EUNSUPPORTED
    assert L.ps_lsh_stage(nv.ptr(A), 64, 32, nv.ptr(img[4:]), nb, st) == nv.PS_EUNSUPPORTED    # not 16-byte aligned
    x = torch.randn(10, 32, device="cuda")
    codes = torch.empty((10, 8), dtype=torch.uint8, device="cuda")
    enc = lambda flags, xp=x, d=32: L.ps_lsh_encode(nv.ptr(xp), 10, d, nv.ptr(img), 64, nv.ptr(codes), flags, st)
    assert enc(nv.PS_LSH_STAGED) == nv.PS_OK
    assert enc(nv.PS_LSH_STAGED | nv.PS_WPERM) == nv.PS_EINVAL
    assert enc(16) == nv.PS_EINVAL
    off = torch.randn(10 * 32 + 4, device="cuda")[1:1 + 10 * 32].view(10, 32)                 # 4 bytes past a 16-byte boundary
    assert enc(nv.PS_LSH_STAGED, off) == nv.PS_EUNSUPPORTED
    assert enc(nv.PS_LSH_STAGED, torch.randn(10, 48, device="cuda"), 48) == nv.PS_EUNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(codes.cpu().numpy(), co.lsh_encode(x.cpu().numpy(), A.cpu().numpy()))
