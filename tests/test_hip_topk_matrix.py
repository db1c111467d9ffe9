"""The top-k selection of the three searches (csrc/dot_topk.hip: WaveSelect under ps_dot_topk, ps_l2_topk plain and masked,
ps_ivf_topk) against an exact oracle, bit for bit.  tests/helpers/topk_cases.py holds the table -- rows that keep improving,
rows that keep worsening, rows of equal values, sweep boundaries inside tie runs, ties that arrive with a smaller id than the keys
already held, more than 64 probed lists, skipped and repeated probes, segments around the 256-element piece -- and
tests/test_topk_cases.py proves on the CPU that each case reaches its situation and that a slip in the selection changes what a
named case expects.  The data is small integers in fp32, so every value the kernels form is exact whatever the summation order:
there is no tolerance anywhere.  Values are compared as int32, ids as int64."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import topk_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = tc.cases()
IVF = [n for n, c in CASES.items() if c.kind == "ivf"]
RANKED = [n for n, c in CASES.items() if c.kind == "dot" and not c.exclude_self]
MULTI = [n for n, c in CASES.items() if c.nq > 1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _launch(c, rows):
    """the case's search over its query rows `rows` (in that order) -> (values fp32 [n, k], ids int64 [n, k]) on the host"""
    from pinsage_hip import dense
    if c.kind == "dot":
        vals, ids = dense.dot_topk(_dev(c.table()), _dev(c.qidx[rows]), c.k, exclude_self=c.exclude_self)
    elif c.kind == "l2":
        vals, ids = dense.l2_topk(_dev(c.table()), _dev(c.queries()[rows]), c.k)
    elif c.kind == "l2m":
        vals, ids = dense.l2_topk(_dev(c.table()), _dev(c.queries()[rows]), c.k, assign=_dev(c.assign),
                                  probe=_dev(tc.probe_bits(c)[rows].view(np.int32)))
    else:
        vals, ids = dense.ivf_topk(_dev(c.table()), _dev(c.list_ptr), _dev(c.item_ids), _dev(c.queries()[rows]),
                                   _dev(c.probes[rows]), c.k, max_list=c.max_list)
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and ids.dtype == torch.int64 and vals.shape == ids.shape == (len(rows), c.k)
    return vals.cpu(), ids.cpu()


@functools.lru_cache(maxsize=None)
def _result(name):
    c = CASES[name]
    return _launch(c, np.arange(c.nq))


def _same(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def _want(c, rows=None):
    vals, ids = tc.oracle(c)
    rows = np.arange(c.nq) if rows is None else rows
    return torch.from_numpy(vals[rows].copy()), torch.from_numpy(ids[rows].copy())


def _report(c, got, want, rows=None):
    """one paragraph per row that differs: the row, the expected and the received (value, id) keys"""
    rows = np.arange(c.nq) if rows is None else rows
    out = []
    for i, r in enumerate(rows):
        g, w = (got[0][i], got[1][i]), (want[0][i], want[1][i])
        if _same(g, w):
            continue
        slot = int(np.flatnonzero((g[0].view(torch.int32) != w[0].view(torch.int32)).numpy() | (g[1] != w[1]).numpy())[0])
        out.append("%s row %d (query value %d): first difference in slot %d\n  expected %s\n  received %s" % (
            c.name, r, c.qval(r), slot, list(zip(w[0].tolist(), w[1].tolist())), list(zip(g[0].tolist(), g[1].tolist()))))
    return "\n".join(out)


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_oracle(name):
    c = CASES[name]
    got, want = _result(name), _want(c)
    assert _same(got, want), _report(c, got, want)


@pytest.mark.parametrize("name", list(CASES))
def test_the_slab_is_the_planted_row(name):
    """dense.linear(E[q], E) -- the GEMM whose rows the selection sweeps -- returns the planted integers exactly, +0.0 for every
    zero: the row order under test is the one the case claims"""
    from pinsage_hip import dense
    c = CASES[name]
    W = _dev(c.table())
    Q = W.index_select(0, _dev(c.qidx)) if c.kind == "dot" else _dev(c.queries())
    slab = dense.linear(Q, W).cpu()
    want = torch.from_numpy(np.stack([c.row_values(r) for r in range(c.nq)]).astype(np.float32))
    assert slab.shape == (c.nq, c.N) and torch.equal(slab.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("name", IVF)
def test_ivf_equals_the_masked_form(name):
    """the header's "identical (dist, ids) to the masked form": ps_l2_topk over the items in original-id order, assign = the list of
    every item, probe bits from the same probes (skipped entries set no bit)"""
    from pinsage_hip import dense
    c = CASES[name]
    x, assign = tc.masked_form(c)
    X = np.zeros((c.N, c.D), dtype=np.float32)
    X[:, 0] = x
    vals, ids = dense.l2_topk(_dev(X), _dev(c.queries()), c.k, assign=_dev(assign), probe=_dev(tc.probe_bits(c).view(np.int32)))
    masked = (vals.cpu(), ids.cpu())
    assert _same(masked, _want(c)), _report(c, masked, _want(c))
    assert _same(_result(name), masked), _report(c, _result(name), masked)


@pytest.mark.parametrize("name", RANKED)
def test_rank_path_agrees(name):
    """dense.target_rank (the rank-count epilogue behind hit rate and MRR) on every emitted slot: item ids[:, r] has rank r + 1,
    through the same ties"""
    from pinsage_hip import dense
    c = CASES[name]
    ids = _result(name)[1]
    assert torch.equal(ids, _want(c)[1])
    r, s = torch.nonzero(ids >= 0, as_tuple=True)
    got = dense.target_rank(_dev(c.table()), torch.from_numpy(c.qidx)[r], ids[r, s]).cpu()
    bad = torch.nonzero(got != s + 1).flatten()[:5].tolist()
    assert not bad, [(c.name, int(r[i]), int(s[i]), int(ids[r[i], s[i]]), int(got[i])) for i in bad]


@pytest.mark.parametrize("name", MULTI)
def test_queries_reversed(name):
    """no row depends on the wave of the workgroup it lands on: the queries in reverse order give the reversed result"""
    c = CASES[name]
    rows = np.arange(c.nq)[::-1].copy()
    got, want = _launch(c, rows), _want(c, rows)
    assert _same(got, want), _report(c, got, want, rows)
    fwd = _result(name)
    assert _same(got, (fwd[0].flip(0), fwd[1].flip(0)))
