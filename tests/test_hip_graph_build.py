"""The sampler graph's device build (csr_build.hip) at a size where every size-gated branch runs, against the C oracle.

The CSR / CDF kernels loop over rows and edges with capped grids: prep_keys / rowptr / gather / pack_edges use at most
8 192 x 256 threads (a second pass once E > 2 097 152), cdf_large_kernel 8 192 waves, guide_build_kernel 16 384 and the
bucket kernels 32 768 (a second pass once V exceeds them), and rocPRIM's radix sort sorts 17 key bits once V > 2^16.  The
graph below has V = 100 008 rows and ~3.7 M edges, rows above 32 edges (the wave-per-row CDF path) all over the id range,
and planted rows on the boundaries that matter: 32 / 33 edges (small / large CDF kernel), 128 / 129 (numpy's pairwise
leaf), 8 192 / 8 193 / 16 392 / 24 577 (numpy's 8 192-element ufunc buffer).  rowptr / col / cdf are compared bit for bit
with the oracle's build from the HOST edge list; the structures derived from them (node records, guide, packed blocks,
both bucket record forms, destination records) with their definitions (tests/helpers/graph_defs.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import bipartite_graph

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from graph_defs import check_graph_definitions  # noqa: E402

pytestmark = pytest.mark.gpu

PLANTED = [32, 33, 128, 129, 8192, 8193, 16392, 3 * 8192 + 1]


def _oracle_threads():
    from oracle import c_oracle as co
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(n, co.max_threads(), 16))


def planted_graph(weights, seed):
    """bipartite_graph's 40 000 items x 60 000 users with 1 750 001 ratings, plus one user per PLANTED degree (ids 100 000 +),
    each rating that many random items (both directions, like every other rating); edges shuffled so the stable sort has
    work to do.  weights: "float" (random fp32, not multiples of 1/2: the summation order shows), "half" or None."""
    M, U, R = 40000, 60000, 1750001                        # E = 3 695 354: not a multiple of 8 (padded packed block)
    ei, ew = bipartite_graph(M, U, R, seed, weights=weights)
    rs = np.random.RandomState(seed + 1)
    users = np.repeat(M + U + np.arange(len(PLANTED)), PLANTED)
    items = rs.randint(0, M, size=users.size)
    ei = np.concatenate([ei, np.stack([users, items]), np.stack([items, users])], axis=1)
    if weights == "half":
        r = rs.randint(1, 11, size=users.size).astype(np.float32) * 0.5
    elif weights == "float":
        r = (rs.random_sample(users.size) * 4.9 + 0.1).astype(np.float32)
    if ew is not None:
        ew = np.concatenate([ew, r, r]).astype(np.float32)
    p = rs.permutation(ei.shape[1])
    return np.ascontiguousarray(ei[:, p]), None if ew is None else np.ascontiguousarray(ew[p])


@pytest.mark.parametrize("weights", ["float", "half", None])
def test_csr_cdf_and_lookup_records_at_multi_pass_size(weights):
    from oracle import c_oracle as co
    from pinsage_hip.graph import DeviceGraph
    ei, ew = planted_graph(weights, seed=11)
    E = ei.shape[1]
    ei_d = torch.from_numpy(ei).cuda()
    ew_d = None if ew is None else torch.from_numpy(ew).cuda()
    g = DeviceGraph(ei_d, ew_d, buckets="full", dest_info=True)
    cg = co.Graph(ei, ew, threads=_oracle_threads())
    # the shape really reaches every second pass (constants of csr_build.hip)
    deg = np.diff(cg.rowptr)
    large = np.nonzero(deg > 32)[0]
    assert E > 8192 * 256 and cg.V > 2 ** 16 and cg.V > 8192 * 4
    for waves in (2048 * 4, 4096 * 4, 8192 * 4):            # cdf_large / guide / bucket kernels: rows on a second pass
        assert np.count_nonzero((large // waves) % 2 == 1) > 1000
    assert np.array_equal(deg[100000:], PLANTED)
    assert g.V == cg.V and g.E == E
    assert np.array_equal(g.rowptr.cpu().numpy(), cg.rowptr)
    assert np.array_equal(g.col.cpu().numpy(), cg.col)
    assert np.array_equal(g.cdf.cpu().numpy().view(np.int64), cg.cdf.view(np.int64))
    assert g.bucket_bytes == 64 and g.dest_info is not None
    check_graph_definitions(g, device="cpu")
    # the default record form (32-byte half records) over the same CSR
    gh = DeviceGraph(ei_d, ew_d, buckets="half")
    assert gh.bucket_bytes == 32 and gh.dest_info is None
    assert torch.equal(gh.rowptr, g.rowptr) and torch.equal(gh.col, g.col)
    assert torch.equal(gh.cdf.view(torch.int64), g.cdf.view(torch.int64))
    check_graph_definitions(gh, device="cpu")


# Five rows of SYN-25M's half-star ratings (digit d = rating 0.5 (d + 1)) whose CDF holds a quotient cdf_i / cdf_last within a
# hair of an fp64 rounding midpoint: the compiler's fp64 division sequence rounded each of them the wrong way (0.7 instead of
# numpy's 0.7000000000000001), one entry per row, until csr_build.hip divided with div_rn.
NEAR_MIDPOINT_ROWS = [
    ("7997883579785535777834956910717793593787499555977662767597697434476733664763577497763795574839738635"
     "866990764563577277594493"),
    ("7765936577757656925797838437688663755459663869767859677475564156655336725466876746615563719776753477"
     "655856757445754573556765743"),
    ("7938954529583335878455982647477765674655576547475598765957597597593967994969985476735587967799868089"
     "4675175677937456863770956785955473556757878679767599679742667776526695637539587775977577856946973969"
     "293987975854779558675599755565398777357849887"),
    ("95689796783770859743365929712596497458355979555795935466593515878655476796773866870797677697777715"),
    ("4983698589595999765778747777577066597673907991739857779977775196657548877143457957757897988758895678"
     "587678074772795775575983678794897737809747974061579996886776977775597757"),
]


def test_cdf_divisions_round_like_numpy_near_a_midpoint():
    """The CDF of each row against numpy itself (p = w / w.sum(); cdf = p.cumsum(); cdf /= cdf[-1]), bit for bit, both as rows
    of the wave-per-row kernel and cut to 32 edges (the lane-per-row kernel)."""
    from pinsage_hip.graph import DeviceGraph
    ws = [(np.array([int(ch) for ch in s]) + 1).astype(np.float32) * np.float32(0.5) for s in NEAR_MIDPOINT_ROWS]
    ws += [w[:32] for w in ws]
    n = len(ws)
    src = np.concatenate([np.full(w.size, r) for r, w in enumerate(ws)])
    dst = np.concatenate([n + np.arange(w.size) for w in ws])
    g = DeviceGraph(torch.from_numpy(np.stack([src, dst])).cuda(), torch.from_numpy(np.concatenate(ws)).cuda(), buckets=False)
    cdf = g.cdf.cpu().numpy()
    rowptr = g.rowptr.cpu().numpy()
    for r, w in enumerate(ws):
        p = w.astype(np.float64) / w.astype(np.float64).sum()
        want = p.cumsum()
        want /= want[-1]
        assert np.array_equal(cdf[rowptr[r]:rowptr[r + 1]].view(np.int64), want.view(np.int64)), r
