"""ps_attention_weights and ps_gather_max (csrc/neigh_agg.hip) over agg_cases.GATE_CASES -- the scalar path's further sweeps, three
slot blocks, nvalid beyond T and below 0, a row whose first slot block keeps nothing -- never against another GPU run:

  attention    +0.0 exactly on every slot that is not kept; the rows with nvalid = T + 5 and 2^31 - 1 equal their twin with
               nvalid = T bit for bit; a row whose kept slots all name one neighbour gets exactly fp32(1 / n); every other weight
               within agg_cases.attention_bound (derived there, about 15 fp32 half-ulps) of the fp64 softmax of the kernel's own
               fp32 scores, which agg_cases.attention_scores_exact restates bit for bit
  gather-max   equality with agg_cases.gather_max_ref, with all-negative features and with a planted NaN and a -inf column"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import agg_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu
GATE_IDS = [f"g{gi}-B{c[0]}-N{c[1]}-C{c[2]}-T{c[3]}" + ("-offset" if c[4] else "") for gi, c in enumerate(ac.GATE_CASES)]


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


@pytest.mark.parametrize("gi", range(len(ac.GATE_CASES)), ids=GATE_IDS)
def test_attention_weights_gates(gi):
    from pinsage_hip import sampling
    c = ac.gate_case(gi)
    o, r, T = c["offset"], c["rows"], c["T"]
    gate = ac.GATE_CASES[gi][5]
    keep = ac.kept(c["raw_ids"], c["nvalid"], c["N"])
    scores = ac.attention_scores_exact(c["u"], c["v"], c["w2"], c["raw_ids"], c["nvalid"], c["vec"])
    ref, bound = ac.softmax_of_scores(scores), ac.attention_bound(scores, T)
    got = sampling.attention_weights(_dev(c["u"], o), _dev(c["v"], o), _dev(c["w2"], o), _dev(c["raw_ids"]), _dev(c["nvalid"]))
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert not got[~keep].view(np.uint32).any(), gate        # exactly +0.0 where nothing is kept: no NaN, no -0.0
    assert not got[r["neg"]].view(np.uint32).any() and not got[r["negmin"]].view(np.uint32).any()
    for name in ("over", "huge"):                             # nvalid beyond T is T
        assert np.array_equal(got[r[name]].view(np.uint32), got[r["twin"]].view(np.uint32)), (gate, name)
    one = keep[r["one"]]
    assert (got[r["one"]][one] == np.float32(1.0) / np.float32(one.sum())).all(), (gate, got[r["one"]][one][:4], one.sum())
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err[keep] / bound[keep]))
    print(f"gate {gi} ({gate}): max |attn - softmax64(exact scores)| / bound = {ratio:.3f}, "
          f"max relative error {np.max(err[keep] / ref[keep]):.3e}, bound {np.max(bound[keep] / ref[keep]):.3e}")
    worst = np.unravel_index(np.argmax(np.where(keep, err - bound, -np.inf)), err.shape)
    assert (err[keep] <= bound[keep]).all(), (gate, ac.agg_facts(c["B"], c["N"], c["C"], T, o), worst, float(got[worst]), float(ref[worst]))
    rows = keep.any(axis=1)
    assert np.array_equal(rows, got.any(axis=1))
    if T > 64:                                                # the late row: its weights sit in the later slot blocks only
        assert not got[r["late"], :64].any() and (got[r["late"], 64:] > 0).all()


@pytest.mark.parametrize("gi", range(len(ac.GATE_CASES)), ids=GATE_IDS)
def test_gather_max_gates(gi):
    from pinsage_hip import sampling
    c = ac.gate_case(gi)
    o, r = c["offset"], c["rows"]
    gate = ac.GATE_CASES[gi][5]
    ids, nvalid = _dev(c["raw_ids"]), _dev(c["nvalid"])
    keep = ac.kept(c["raw_ids"], c["nvalid"], c["N"])
    x = -np.abs(c["x"]) - 1.0                               # all negative: a maximum started from 0 would show
    got = sampling.gather_max(_dev(x, o), ids, nvalid).cpu().numpy()
    ref = ac.gather_max_ref(x, c["raw_ids"], c["nvalid"])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (gate, np.argwhere(got != ref)[:6])
    assert (ref[keep.any(axis=1)] < 0).all() and not ref[~keep.any(axis=1)].any()
    assert not got[r["neg"]].view(np.uint32).any() and not got[r["negmin"]].view(np.uint32).any()
    assert np.array_equal(got[r["over"]], got[r["twin"]]) and np.array_equal(got[r["huge"]], got[r["twin"]])
    if c["T"] > 64:
        assert (got[r["late"]] < 0).all()                     # found beyond the first slot block
    x = x.copy()
    i, j = np.argwhere(keep)[-1]
    x[c["raw_ids"][i, j], 0] = np.nan                       # a gathered NaN
    x[:, c["C"] - 1] = -np.inf                              # a column whose maximum is -inf
    got = sampling.gather_max(_dev(x, o), ids, nvalid).cpu().numpy()
    ref = ac.gather_max_ref(x, c["raw_ids"], c["nvalid"])
    assert np.isnan(ref[i, 0]) and np.isneginf(ref[i, -1])
    assert np.array_equal(got, ref, equal_nan=True), gate
    if c["T"] > 64:                                           # a NaN met only in the third slot block stays
        x[:, 0] = -1.0
        late = c["raw_ids"][r["late"]]
        x[late[c["T"] - 1], 0] = np.nan
        got = sampling.gather_max(_dev(x, o), ids, nvalid).cpu().numpy()
        ref = ac.gather_max_ref(x, c["raw_ids"], c["nvalid"])
        assert np.isnan(ref[r["late"], 0]) and np.array_equal(got, ref, equal_nan=True), gate
