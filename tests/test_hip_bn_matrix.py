"""ps_bn_batch_stats and ps_bn_apply (csrc/batch_norm.hip) over the gate table of tests/helpers/bn_cases.py, against its exact
restatements -- never an fp64 reference with a tolerance, never another GPU run:

  statistics   the caller's workspace equals the restated partial sums bit for bit; mean, var, scale and the running statistics
               equal the restated fp32 values (every column is decided: tests/test_bn_cases.py); the same bits on a second call
               and from a workspace full of 0xFF bytes; nothing written past ps_bn_stats_workspace_bytes
  apply        bit equality with the restatement with ReLU on and off, with and without the row norm, out of place and in
               place, planted all-negative and NaN rows included.  With the norm this rests on fp32 sqrt and division being
               correctly rounded in this build (no fast-math flag); tests/test_bn_cases.py tells the summation order from its
               near misses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bn_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a, offset=0):
    """a on the device; offset: that many elements into its storage (contiguous, not 16-byte aligned for one float)"""
    a = np.ascontiguousarray(a)
    if not offset:
        t = torch.tensor(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + offset, dtype=torch.tensor(a[:0]).dtype, device="cuda")
    t = buf[offset:].view(a.shape)
    t.copy_(torch.tensor(a))
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t


def _stats(z, gamma, rm, rv, ws, wsb):
    """ps_bn_batch_stats with a workspace of the caller's; returns (mean, var, scale)"""
    from pinsage_hip import native as nv
    M, N = z.shape
    mean, var, scale = (torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(3))
    rc = nv.lib().ps_bn_batch_stats(nv.ptr(z), M, N, nv.ptr(gamma), bc.EPS, bc.MOMENTUM, nv.ptr(rm), nv.ptr(rv), nv.ptr(mean),
                                    nv.ptr(var), nv.ptr(scale), nv.ptr(ws), wsb, nv.stream())
    assert rc == nv.PS_OK
    return mean, var, scale


@pytest.mark.parametrize("name", bc.STATS_NAMES)
def test_bn_batch_stats_bits(name):
    from pinsage_hip import native as nv
    case = bc.stats_case(name)
    f = bc.facts(case)
    d, want = bc.stats_data(name), bc.stats_expected(name)
    M, N = d["M"], d["N"]
    assert all(want["decided"][k].all() for k in bc.OUTPUTS)
    z, gamma, rm, rv = _dev(d["z"], case[3]), _dev(d["gamma"]), _dev(d["rm0"]), _dev(d["rv0"])
    wsb = nv.lib().ps_bn_stats_workspace_bytes(M, N)
    assert wsb == f["workspace_bytes"]
    ws = torch.zeros(wsb + 64, dtype=torch.uint8, device="cuda")
    mean, var, scale = _stats(z, gamma, rm, rv, ws, wsb)
    part = ws[:wsb].cpu().numpy().view(np.float64).reshape(f["P"], 2, N)
    bad = np.argwhere(part.view(np.uint64) != want["part"].view(np.uint64))
    assert not bad.size, (name, case[4], f, [(tuple(b), float(part[tuple(b)]), float(want["part"][tuple(b)])) for b in bad[:6]])
    got = {"mean": mean, "var": var, "scale": scale, "rm": rm, "rv": rv}
    for k in bc.OUTPUTS:
        bad = bc.mismatches(got[k].cpu().numpy(), want[k])
        assert not bad, (name, k, case[4], f, bad)
    assert not ws[wsb:].any()                                 # nothing is written past the workspace's size
    # the same bits again, and once more from a workspace full of 0xFF bytes (NaNs, as doubles); no running pointers: no update
    ws2 = torch.full((wsb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    for w in (ws, ws2):
        again = _stats(z, gamma, None, None, w, wsb)
        assert all(torch.equal(a, b) for a, b in zip(again, (mean, var, scale))), name
    assert torch.equal(ws2[:wsb], ws[:wsb]) and (ws2[wsb:] == 0xFF).all()
    assert not bc.mismatches(rm.cpu().numpy(), want["rm"]) and not bc.mismatches(rv.cpu().numpy(), want["rv"])


@pytest.mark.parametrize("name", bc.APPLY_NAMES)
def test_bn_apply_bits(name):
    from pinsage_hip import dense
    case = bc.apply_case(name)
    f = bc.facts(case)
    d = bc.apply_data(name)
    z = _dev(d["z"], case[3])
    mean, scale, beta = _dev(d["mean"]), _dev(d["scale"]), _dev(d["beta"], case[4])
    for relu in (False, True):
        for l2 in (False, True):
            want = bc.apply_exact(d["z"], d["mean"], d["scale"], d["beta"], relu, l2, f["vec"])
            out = dense.batch_norm_apply(z, mean, scale, beta, relu, l2)
            got = out.cpu().numpy()
            bad = bc.mismatches(got, want)
            if bad and l2:                                    # where does it part: before the norm, or in the sqrt / division?
                pre = bc.prenorm_exact(d["z"], d["mean"], d["scale"], d["beta"], relu).astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ref = pre / np.maximum(np.sqrt((pre * pre).sum(axis=1, keepdims=True)), 1e-12)
                    rel = np.nanmax(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))
                print(f"{name} relu {relu}: {len(bad)}+ mismatches, max relative distance from the fp64 norm of the exact pre-norm values {rel:.3e}")
            assert not bad, (name, case[5], f, dict(relu=relu, l2=l2), bad)
            z2 = _dev(d["z"], case[3])
            assert dense.batch_norm_apply(z2, mean, scale, beta, relu, l2, out=z2) is z2
            bad = bc.mismatches(z2.cpu().numpy(), want)       # in place: the bits of out of place, on the long-row path too
            assert not bad, (name, case[5], f, dict(relu=relu, l2=l2, in_place=True), bad)
            if d["neg_row"] is not None:
                row = got[d["neg_row"]]
                if relu:                                      # +0.0 throughout, through the 1e-12 clamp of the norm too
                    assert not row.view(np.uint32).any()
                else:
                    assert (row < 0).all()
                nan = np.isnan(got)
                assert nan.sum() == (d["N"] if l2 else 1) and nan[d["nan_row"], -1]
    assert not bc.mismatches(z.cpu().numpy(), np.ascontiguousarray(d["z"]))                  # out of place leaves z alone
