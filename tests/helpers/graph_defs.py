"""Vectorised restatements of the sampler graph's lookup structures (csr_build.hip, include/pinsage_hip.h), checked
against a built DeviceGraph.  Every check is a whole-array torch expression in fp64 / integer arithmetic on whatever device
the graph lives on -- no Python loop per edge -- so the same code runs on a 3 M-edge test graph and on SYN-25M's 50 M
edges.  The CSR / CDF themselves are held to the C oracle elsewhere; these checks take them as given and restate what
is derived from them."""
import torch

GUIDE_SHRINK = 1.0 - 2.0 ** -50          # guide_build_kernel: t = (j / deg) * (1 - 2^-50)


def _edge_rows(rowptr):
    """(row of every edge, that row's first edge, that row's end) as int64 vectors"""
    deg = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(deg.numel(), device=rowptr.device), deg)
    return row, rowptr[row], rowptr[row + 1]


def expected_guide(rowptr, cdf):
    """guide[lo + j] = #{k : cdf[lo + k] <= (j / deg) * (1 - 2^-50)}, 0 for j = 0: a bisection of every row at once, with the
    threshold computed by the kernel's expression (two IEEE fp64 operations, so bit-identical)."""
    E = cdf.numel()
    row, lo, hi = _edge_rows(rowptr)
    j = torch.arange(E, device=cdf.device) - lo
    t = (j.double() / (hi - lo).double()) * GUIDE_SHRINK
    l, h = lo.clone(), hi.clone()
    h[j == 0] = lo[j == 0]
    steps = int((hi - lo).max().item()).bit_length() + 1 if E else 0
    for _ in range(steps):                                  # invariant: cdf[lo:l] <= t < cdf[h:hi]
        act = l < h
        mid = l + ((h - l) >> 1)
        le = cdf[mid.clamp(max=max(E - 1, 0))] <= t
        l = torch.where(act & le, mid + 1, l)
        h = torch.where(act & ~le, mid, h)
    assert bool((l == h).all())
    return (h - lo).to(torch.int32)


def candidates(rowptr, col, cdf, guide, n):
    """The n CDF entries / destinations from every edge's guide position on, as the bucket records hold them: past the row end
    the entry is 2.0 and the destination the row's last edge."""
    row, lo, hi = _edge_rows(rowptr)
    idx = (lo + guide.long())[:, None] + torch.arange(n, device=cdf.device)[None, :]
    last = hi[:, None] - 1
    c = torch.where(idx <= last, cdf[torch.minimum(idx, last)], torch.full_like(cdf[:1], 2.0))
    k = col[torch.minimum(idx, last)]
    return c.contiguous(), k


def round_down_f32(c):
    """bucket_half_build_kernel's round_down_f32: round to the nearest fp32, then step one ulp down if that went up (c > 0:
    positive floats order like their bits)."""
    f = c.to(torch.float32)
    fb = f.view(torch.int32)
    return torch.where(f.double() > c, fb - 1, fb).view(torch.float32)


def expected_full_buckets(rowptr, col, cdf, guide):
    """64-byte records [c0 c1 | c2 c3 | k0 k1 k2 k3 | c4 k4 0] as int32 words [E, 16]"""
    c, k = candidates(rowptr, col, cdf, guide, 5)
    cw = c.view(torch.int32)                                # [E, 10]: c_i = words 2i, 2i + 1
    return torch.cat([cw[:, :8], k[:, :4], cw[:, 8:10], k[:, 4:5], torch.zeros_like(k[:, :1])], dim=1)


def expected_half_buckets(rowptr, col, cdf, guide):
    """32-byte records [c0 c1 c2 c3 | k0 k1 k2 k3] (c rounded down to fp32) as int32 words [E, 8]"""
    c, k = candidates(rowptr, col, cdf, guide, 4)
    return torch.cat([round_down_f32(c).view(torch.int32), k], dim=1)


def expected_packed(col, cdf, guide):
    """128-byte blocks of 8 edges: 8 x fp64 cdf | 8 x int32 col | 8 x int32 guide, the tail padded with (2.0, -1, 0)"""
    E = col.numel()
    P = (E + 7) // 8 * 8
    c = torch.full((P,), 2.0, dtype=torch.float64, device=cdf.device)
    k = torch.full((P,), -1, dtype=torch.int32, device=col.device)
    g = torch.zeros(P, dtype=torch.int32, device=col.device)
    c[:E], k[:E], g[:E] = cdf, col, guide
    return torch.cat([c.view(-1, 8).view(torch.uint8), k.view(-1, 8).view(torch.uint8), g.view(-1, 8).view(torch.uint8)], dim=1)


def check_graph_definitions(g, device=None):
    """Assert that every structure a DeviceGraph derives from its CSR / CDF (node records, guide, packed blocks, bucket
    records of either form, destination records) matches its definition, and that compact() + expand() give back the same
    bits.  device: where to evaluate the restatements (None: the graph's device)."""
    dev = g.device if device is None else torch.device(device)
    rowptr, col, cdf = g.rowptr.to(dev), g.col.to(dev), g.cdf.to(dev)
    V, E = g.V, g.E
    ni = g.nodeinfo.to(dev).view(V, 2)                      # (first edge, degree)
    assert torch.equal(ni[:, 0].long(), rowptr[:-1]) and torch.equal(ni[:, 1].long(), rowptr[1:] - rowptr[:-1]), "node records"
    guide = expected_guide(rowptr, cdf)
    assert torch.equal(g.guide.to(dev), guide), "guide"
    assert torch.equal(g.packed.to(dev).view(-1, 128), expected_packed(col, cdf, guide)), "packed blocks"
    if g.buckets is not None:
        words = g.buckets.to(dev).view(torch.int32).view(E, g.bucket_bytes // 4)
        make = expected_full_buckets if g.bucket_bytes == 64 else expected_half_buckets
        assert torch.equal(words, make(rowptr, col, cdf, guide)), f"{g.bucket_bytes}-byte bucket records"
        del words
    if g.dest_info is not None:
        assert torch.equal(g.dest_info.to(dev).view(E, 2), ni[col.long()]), "destination records"
    col0, cdf0, guide0 = g.col.clone(), g.cdf.clone(), g.guide.clone()
    g.compact()
    assert g.col is None and g.cdf is None and g.guide is None
    g.expand()
    assert torch.equal(g.col, col0) and torch.equal(g.guide, guide0)
    assert torch.equal(g.cdf.view(torch.int64), cdf0.view(torch.int64))
