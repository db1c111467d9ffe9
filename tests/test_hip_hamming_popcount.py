"""The popcount Hamming scan (csrc/hamming_topk.hip: hamming_scan_kernel + the slice merge kernels) at the shapes it serves
alone, where the fp4-MFMA scan cannot be the second opinion: 1024-bit codes (cs = 128: the only G = 2 instantiation, key
shift 21), 32 < k <= 64 (the sorted list fills the whole wave), a code table that is 4- but not 16-byte aligned (scalar item
loads), the 32-query tile of tables >= 256 MiB, tables smaller than a wave / than k / empty, and ids beyond 2^32 through the
slice merge.  Everything is integer arithmetic: (distance, id) lists must equal, bit for bit,

  * the C oracle (oracle.c_oracle.hamming_topk: faiss' hammings_knn_hc restated), ids shifted by id_offset, positions past
    min(k, N) forced to the (INT32_MAX, -1) padding, and
  * a numpy restatement (np.unpackbits of the XOR, summed; np.lexsort by (distance, id)), so that the oracle is not the only
    witness at cs = 128 and k = 64.  tests/test_c_oracle.py holds the two references to each other without a GPU.

Every table carries copies of one code at item 0, at the last item and 63 / 64 / 65 items from either end (the edges of a
wave's 64-item group); that code is query 0.  Data kinds: "random", "few" (50 distinct codes: long runs of equal distance
where only the id decides), "same" (one code: the answer is ids 0..k-1 and only the strict-less admission matters).

Not reached here: the minimum-slice rule `smin` of pick_splits binds only when ceil(4096 / query tiles) falls below
ceil(N / 2^key_shift), i.e. with more than about 131 000 queries against a table of more than 2^21 items -- minutes of
oracle time, not a test of a few seconds, so no shape pretends to cover it."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT_MAX = 0x7fffffff
KINDS = ("random", "few", "same")


# ---------------------------------------------------------------------------------------------------------------------
# references and data (numpy only: tests/test_c_oracle.py imports them on machines without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def np_hamming_topk(q, codes, k):
    """k smallest by (distance, id), ascending, ids from 0; (INT32_MAX, -1) past min(k, N).  -> (int32 [nq, k], int64 [nq, k])"""
    nq, N = q.shape[0], codes.shape[0]
    dist = np.full((nq, k), INT_MAX, dtype=np.int32)
    ids = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, N)
    if kk == 0 or nq == 0:
        return dist, ids
    all_ids = np.arange(N, dtype=np.int64)
    rows = max(1, (32 << 20) // (N * codes.shape[1] * 8))            # queries per block: at most 32 MiB of unpacked bits
    for lo in range(0, nq, rows):
        d = np.unpackbits(q[lo:lo + rows, None, :] ^ codes[None, :, :], axis=-1).sum(-1, dtype=np.int32)
        for r in range(d.shape[0]):
            order = np.lexsort((all_ids, d[r]))[:kk]
            dist[lo + r, :kk] = d[r, order]
            ids[lo + r, :kk] = order
    return dist, ids


def cut_and_offset(ref, k, id_offset):
    """the first k columns of a reference computed for a larger k (a (distance, id) order has the prefix property), ids moved
    by id_offset, padding kept"""
    d, i = ref[0][:, :k].copy(), ref[1][:, :k].copy()
    i[i >= 0] += id_offset
    return d, i


def oracle_hamming_topk(q, codes, k, id_offset=0):
    """the C oracle's answer in the kernel's types: int32 distances, ids + id_offset, exact padding past min(k, N)"""
    from oracle import c_oracle as co
    rd, ri = co.hamming_topk(q, codes, k, threads=8)
    kk = min(k, codes.shape[0])
    assert (ri[:, :kk] >= 0).all()
    dist = np.full(rd.shape, INT_MAX, dtype=np.int32)
    ids = np.full(ri.shape, -1, dtype=np.int64)
    dist[:, :kk] = rd[:, :kk].astype(np.int32)
    ids[:, :kk] = ri[:, :kk] + id_offset
    return dist, ids


def plant_positions(N):
    """item 0, the last item, 63 / 64 / 65 items from either end"""
    return sorted(p for p in {0, N - 1, 63, 64, 65, N - 64, N - 65, N - 66} if 0 <= p < N)


def make_case(cs, N, nq, kind, seed):
    """-> (q uint8 [nq, cs], codes uint8 [N, cs], planted positions).  Queries are table codes, every other one with up to
    three bits flipped, every fourth one replaced by a random code; query 0 is the planted code."""
    rs = np.random.RandomState(seed)
    if kind == "random":
        codes = rs.randint(0, 256, size=(N, cs)).astype(np.uint8)
    elif kind == "few":
        codes = rs.randint(0, 256, size=(50, cs)).astype(np.uint8)[rs.randint(0, 50, size=N)]
    elif kind == "same":
        codes = np.tile(rs.randint(0, 256, size=(1, cs)).astype(np.uint8), (N, 1))
    else:
        raise ValueError(kind)
    planted = codes[0].copy() if (kind == "same" and N) else rs.randint(0, 256, size=cs).astype(np.uint8)
    pos = plant_positions(N)
    codes[pos] = planted
    q = codes[rs.randint(0, N, size=nq)].copy() if N else rs.randint(0, 256, size=(nq, cs)).astype(np.uint8)
    for r in range(1, nq, 2):
        for b in rs.randint(0, cs * 8, size=rs.randint(1, 4)):
            q[r, b >> 3] ^= np.uint8(1 << (b & 7))
    q[2::4] = rs.randint(0, 256, size=q[2::4].shape).astype(np.uint8)
    q[0] = planted
    return np.ascontiguousarray(q), np.ascontiguousarray(codes), pos


# ---------------------------------------------------------------------------------------------------------------------
def _popcount_scan(qt, ct, k, id_offset=0):
    from pinsage_hip import dense
    d, i = dense.hamming_topk(qt, ct, k, id_offset=id_offset, use_mfma=False)
    assert d.dtype == torch.int32 and i.dtype == torch.int64 and tuple(d.shape) == tuple(i.shape) == (int(qt.size(0)), k)
    return d, i


def _assert_lists(got, want, what):
    d, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(d, want[0]), (what, "distances")
    assert np.array_equal(i, want[1]), (what, "ids")


def _check_all_k(cs, N, nq, kind, ks, offsets, seed):
    """one data set, every k: the kernel against the numpy restatement (computed once for k = 64) and the oracle (per k)"""
    q, codes, pos = make_case(cs, N, nq, kind, seed)
    ref64 = np_hamming_topk(q, codes, 64)
    qt, ct = torch.from_numpy(q).cuda(), torch.from_numpy(codes).cuda()
    for k, off in zip(ks, offsets):
        what = dict(cs=cs, N=N, nq=nq, kind=kind, k=k, id_offset=off)
        got = _popcount_scan(qt, ct, k, off)
        _assert_lists(got, cut_and_offset(ref64, k, off), (what, "numpy"))
        _assert_lists(got, oracle_hamming_topk(q, codes, k, off), (what, "oracle"))
        # query 0 is the planted code: its copies lead the list in id order ("same": every item is a copy)
        lead = (list(range(N)) if kind == "same" else pos)[:k]
        assert got[1][0, :len(lead)].tolist() == [p + off for p in lead], what
        assert int(got[0][0, :len(lead)].abs().sum()) == 0, what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nq", [5, 67])
@pytest.mark.parametrize("N", [1000, 4100, 20011])
def test_1024_bit_codes(N, nq, kind):
    """a. cs = 128: hamming_scan_kernel<32, 2>, never the MFMA scan.  N = 20011 runs 15 or 16 slices, so k = 33 and
    64 (P * k > 256) go through the wave-per-query merge and k = 1, 11 through the 16-lane selection; ids carry offsets
    beyond 2^32 through both."""
    from pinsage_hip import dense
    ks = (1, 11, 33, 64)
    for k in ks:
        assert not dense.hamming_mfma_supported(nq, N, 128, k)
    _check_all_k(128, N, nq, kind, ks, (0, 2 ** 32 + 1, 2 ** 35 + 9, 2 ** 33 + 5), seed=N * 7 + nq)


@pytest.mark.parametrize("N,kind", [(3000, "random"), (700, "few")])
@pytest.mark.parametrize("cs", [4, 8, 16, 32, 64, 128])
def test_kcap_ladder(cs, N, kind):
    """b. the list capacity kcap = 16 / 32 / 64 on both sides of each step, at every code size: k = 16 | 17, 32 | 33, 63 | 64
    (at kcap = 64 every lane holds a list entry and the bound is read from lane k - 1 = 62 or 63)"""
    ks = (16, 17, 32, 33, 63, 64)
    _check_all_k(cs, N, 9, kind, ks, [2 ** 32 + k for k in ks], seed=cs * 31 + N)


@pytest.mark.parametrize("N", [0, 1, 2, 63, 64, 65, 255, 257])
@pytest.mark.parametrize("cs", [4, 32, 128])
def test_tiny_tables_and_ragged_tiles(cs, N):
    """c. tables of less than / exactly / just over one 64-item group and one G-group chunk, an empty table (NULL codes
    pointer), N < k (unfilled list entries must come out as (INT32_MAX, -1), nothing else), and 1 / 3 / 5 queries against the
    tile of 4"""
    for kind in KINDS:
        q, codes, _ = make_case(cs, N, 5, kind, seed=cs * 1000 + N)
        ref64 = np_hamming_topk(q, codes, 64)
        qt, ct = torch.from_numpy(q).cuda(), torch.from_numpy(codes).cuda()
        for nq in (1, 3, 4, 5):
            for k in (1, 5, 40, 64):
                off = 2 ** 34 + 1 if k in (5, 64) else 0
                what = dict(cs=cs, N=N, nq=nq, kind=kind, k=k, id_offset=off)
                d, i = _popcount_scan(qt[:nq], ct, k, off)
                _assert_lists((d, i), cut_and_offset((ref64[0][:nq], ref64[1][:nq]), k, off), (what, "numpy"))
                _assert_lists((d, i), oracle_hamming_topk(q[:nq], codes, k, off), (what, "oracle"))
                d, i = d.cpu().numpy(), i.cpu().numpy()
                kk = min(k, N)
                assert np.all(d[:, kk:] == INT_MAX) and np.all(i[:, kk:] == -1), what
                assert np.all(i[:, :kk] >= off) and np.all(i < N + off), what
                assert np.all(d[:, :kk] <= cs * 8), what


@pytest.mark.parametrize("k", [11, 40])
@pytest.mark.parametrize("cs", [16, 32, 64, 128])
def test_table_base_not_16_byte_aligned(cs, k):
    """d. WORDS % 4 == 0 but the table starts 4 bytes into a 16-byte line: the item loads take the dword branch instead of the
    16-byte one.  dense.hamming_topk passes an offset contiguous view through unchanged, so the kernel sees that pointer.  Same
    for the (scalar-loaded) queries."""
    N, nq, off = 5003, 37, 2 ** 32 + 3
    for kind in ("random", "few"):
        q, codes, _ = make_case(cs, N, nq, kind, seed=cs + k)
        qt, ct = torch.from_numpy(q).cuda(), torch.from_numpy(codes).cuda()
        assert ct.data_ptr() % 16 == 0 and qt.data_ptr() % 16 == 0
        cbuf = torch.zeros(4 + N * cs + 12, dtype=torch.uint8, device="cuda")
        qbuf = torch.zeros(4 + nq * cs + 12, dtype=torch.uint8, device="cuda")
        cu, qu = cbuf[4:4 + N * cs].view(N, cs), qbuf[4:4 + nq * cs].view(nq, cs)
        cu.copy_(ct)
        qu.copy_(qt)
        for t in (cu, qu):
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        want_np = cut_and_offset(np_hamming_topk(q, codes, k), k, off)
        want_c = oracle_hamming_topk(q, codes, k, off)
        aligned = _popcount_scan(qt, ct, k, off)
        for name, (qq, cc) in (("aligned", (qt, ct)), ("table+4", (qt, cu)), ("table+4, queries+4", (qu, cu))):
            what = dict(cs=cs, k=k, kind=kind, case=name)
            got = _popcount_scan(qq, cc, k, off)
            assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1]), what
            _assert_lists(got, want_np, (what, "numpy"))
            _assert_lists(got, want_c, (what, "oracle"))


BIG_N, BIG_CS, BIG_NQ = (1 << 21) + 77, 128, 33


@pytest.fixture(scope="module")
def big_table():
    """a 1024-bit table just over 256 MiB, made on the device and copied to the host once for the oracle"""
    g = torch.Generator(device="cuda").manual_seed(1024)
    ct = torch.randint(0, 256, (BIG_N, BIG_CS), dtype=torch.uint8, device="cuda", generator=g)
    planted = torch.randint(0, 256, (BIG_CS,), dtype=torch.uint8, device="cuda", generator=g)
    pos = [0, 1 << 20, BIG_N - 1]
    ct[pos] = planted
    # queries: table codes from both ends, slice edges and the middle; odd ones with a few bits flipped; query 0 = planted
    rows = (torch.arange(BIG_NQ, dtype=torch.int64) * (BIG_N - 1) // (BIG_NQ - 1)).cuda()      # 0 ... N - 1, evenly
    qt = ct[rows].clone()
    flip = torch.zeros_like(qt)
    flip[1::2, ::17] = 0x21
    qt ^= flip
    qt[0] = planted
    codes = ct.cpu().numpy()
    yield qt.contiguous(), ct, qt.cpu().numpy(), codes, pos
    del ct


@pytest.mark.parametrize("k", [11, 64])
def test_32_query_tile_over_256_mib(big_table, k):
    """e. N * cs >= 256 MiB switches the scan to 32 queries per wave: 32 KiB of lists per block at kcap = 64, admission bounds
    in lanes 0..31, 33 queries = one full and one ragged tile (one query), 1024 slices merged by the wave-per-query kernel, and
    N > 2^21 = 2^key_shift(128) items, so a single slice could not hold the local ids.  Oracle only: the numpy restatement would
    unpack 2 GiB per query.  Both k stay: the oracle needs well under a second for each."""
    from pinsage_hip import dense
    qt, ct, q, codes, pos = big_table
    assert BIG_N * BIG_CS >= 256 << 20 and tuple(ct.shape) == (BIG_N, BIG_CS)          # on the far side of pick_tile's gate
    assert not dense.hamming_mfma_supported(BIG_NQ, BIG_N, BIG_CS, k)
    off = 2 ** 33 + 5
    t0 = time.perf_counter()
    want = oracle_hamming_topk(q, codes, k, off)
    t1 = time.perf_counter()
    got = _popcount_scan(qt, ct, k, off)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"32-query tile, k = {k}: oracle {t1 - t0:.2f} s, scan + merge {t2 - t1:.3f} s")
    _assert_lists(got, want, dict(k=k))
    lead = pos[:k]
    assert got[1][0, :len(lead)].tolist() == [p + off for p in lead] and int(got[0][0, :len(lead)].abs().sum()) == 0
    # the ragged tile's only query is the table's last code = the planted one: the same list as query 0 of the full tile
    assert np.array_equal(q[BIG_NQ - 1], q[0])
    assert torch.equal(got[0][BIG_NQ - 1], got[0][0]) and torch.equal(got[1][BIG_NQ - 1], got[1][0])
