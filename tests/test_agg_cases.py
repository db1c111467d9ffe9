"""The attention / max-pool aggregator cases without a GPU: the float64 restatement of tests/helpers/agg_cases.py reproduces the
reference's recorded outputs (G4 of reference_golden.npz and reference_golden_agg.npz), the case inputs are fair -- the
reference's formula in plain fp32 torch on the CPU stays inside the tolerance the HIP path is held to -- the modules' torch
path (CPU tensors) still equals the goldens, and the two C entry points keep their argument rules."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import agg_cases as ac  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G4_NBRS = [[1, 2, 3], [], [0], [4, 5, 6, 7, 8], [9, 10], [11, 0, 1]]
CASE_IDS = [f"{ci}-B{c[0]}-N{c[1]}-C{c[2]}-T{c[3]}" for ci, c in enumerate(ac.CASES)]


@pytest.fixture(scope="module")
def golden_agg():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_golden_agg.npz"))


def _golden_lists(g):
    return [[int(t) for t in g["ids"][i, :g["nvalid"][i]]] for i in range(g["ids"].shape[0])]


def _load(module, g, prefix):
    sd = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
    assert set(sd) == set(module.state_dict())
    module.load_state_dict(sd)
    return module.eval()


def test_restatement_reproduces_the_goldens(golden, golden_agg):
    """to 1e-12 against the reference run on the goldens cast to float64 (recorded by make_golden_agg.py), and to fp32 rounding
    against the fp32 outputs the goldens hold"""
    g, a = golden, golden_agg
    f = g["g4_features"]
    got = ac.attention_forward_ref(f, G4_NBRS, g["g4_at_attention.0.weight"], g["g4_at_attention.0.bias"],
                                   g["g4_at_attention.2.weight"], g["g4_at_attention.2.bias"])
    np.testing.assert_allclose(got, a["g4_attention64"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, g["g4_attention"].astype(np.float64), rtol=1e-5, atol=1e-6)
    got = ac.maxpool_forward_ref(f, G4_NBRS, g["g4_mp_mlp.0.weight"], g["g4_mp_mlp.0.bias"])
    np.testing.assert_allclose(got, a["g4_maxpool64"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, g["g4_maxpool"].astype(np.float64), rtol=1e-5, atol=1e-6)
    nb = _golden_lists(a)
    got = ac.attention_forward_ref(a["features"], nb, a["at_attention.0.weight"], a["at_attention.0.bias"],
                                   a["at_attention.2.weight"], a["at_attention.2.bias"], a["self_features"])
    np.testing.assert_allclose(got, a["attention64"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, a["attention"].astype(np.float64), rtol=ac.RTOL, atol=ac.ATOL)
    got = ac.maxpool_forward_ref(a["features"], nb, a["mp_mlp.0.weight"], a["mp_mlp.0.bias"])
    np.testing.assert_allclose(got, a["maxpool64"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, a["maxpool"].astype(np.float64), rtol=ac.RTOL, atol=ac.ATOL)


def test_split_first_layer_is_the_same_formula():
    """cat([self, nbr]) W1^T + b1 = (self W1[:, :C]^T + b1) + nbr W1[:, C:]^T, and the last layer's bias drops out of the softmax:
    the raw entry point's restatement over u / v / w2 gives the module restatement's output (float64, 1e-12)"""
    for ci in (2, 3, 6):
        c = ac.case(ci)
        at, _ = ac.modules(ci)
        p = {k: t.detach().numpy().astype(np.float64) for k, t in at.state_dict().items()}
        C = c["C"]
        W1 = p["attention.0.weight"]
        u = c["self_x"].astype(np.float64) @ W1[:, :C].T + p["attention.0.bias"]
        v = c["x"].astype(np.float64) @ W1[:, C:].T
        attn = ac.attention_weights_ref(u, v, p["attention.2.weight"][0], c["ids"], c["nvalid"])
        out = np.einsum("bt,btc->bc", attn, c["x"].astype(np.float64)[np.maximum(c["ids"], 0)])
        np.testing.assert_allclose(out, ac.at_ref(at, c["x"], c["neighbors"], c["self_x"]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("ci", range(len(ac.CASES)), ids=CASE_IDS)
def test_case_inputs_are_fair(ci):
    """the torch code the HIP path replaces, in fp32 on the CPU, is inside the HIP path's tolerance on every case: the cases ask
    nothing of fp32 that the formula's straightforward evaluation does not deliver"""
    c = ac.case(ci)
    x, sx = torch.tensor(c["x"]), torch.tensor(c["self_x"])
    for scaled in ((False, True) if ci == ac.SCALED_CASE else (False,)):
        at, mp = ac.modules(ci, scaled)
        with torch.no_grad():
            got = at._forward_torch(x, c["neighbors"], sx).numpy()
            ref = ac.at_ref(at, c["x"], c["neighbors"], c["self_x"])
            print(f"case {ci} scaled {scaled}: attention max |fp32 - fp64| {np.abs(got - ref).max():.2e} on values up to {np.abs(ref).max():.2f}")
            np.testing.assert_allclose(got, ref, rtol=ac.RTOL, atol=ac.ATOL)
            got = mp._forward_torch(x, c["neighbors"]).numpy()
            np.testing.assert_allclose(got, ac.mp_ref(mp, c["x"], c["neighbors"]), rtol=ac.RTOL, atol=ac.ATOL)
    # the raw operands: fp32 scores and softmax against the float64 restatement
    u, v, w2 = (torch.tensor(c[k]) for k in ("u", "v", "w2"))
    keep = ac.kept(c["raw_ids"], c["nvalid"], c["N"])
    idt = torch.from_numpy(np.where(keep, c["raw_ids"], 0).astype(np.int64))
    for scale in ((1.0, 8.0) if ci == ac.SCALED_CASE else (1.0,)):
        s = (torch.relu(u[:, None, :] + v[idt]) * (w2 * scale)).sum(dim=2).masked_fill(~torch.from_numpy(keep), float("-inf"))
        attn = torch.nan_to_num(torch.softmax(s, dim=1), nan=0.0).numpy()             # a row that keeps nothing: softmax of all -inf
        np.testing.assert_allclose(attn, ac.attention_weights_ref(c["u"], c["v"], c["w2"] * np.float32(scale), c["raw_ids"], c["nvalid"]),
                                   rtol=ac.RTOL, atol=ac.ATOL)


def test_case_table_covers_what_it_says():
    for ci, (B, N, C, T, _) in enumerate(ac.CASES):
        c = ac.case(ci)
        nv = c["nvalid"]
        assert nv[0] == 1 and (B < 4 or {0, 1, T} <= set(nv.tolist()))
        keep = ac.kept(c["raw_ids"], nv, N)
        if ci == 0:
            assert keep.all()
        else:
            inrow = np.arange(T)[None, :] < nv[:, None]
            assert np.array_equal(ac.kept(c["ids"], nv, N), inrow)                          # the module-legal ids keep every slot
            if B > 6:
                assert {-1, N, 2 ** 31 - 1} <= set(c["raw_ids"][inrow].tolist())
                assert ((nv > 0) & ~keep.any(axis=1)).any()                                 # a row with slots that keeps nothing
        if T >= 2:                                                                          # duplicate ids within a row
            assert any(len(set(nb)) < len(nb) for nb in c["neighbors"])


def test_modules_on_cpu_tensors_equal_the_goldens(golden, golden_agg):
    """CPU tensors take the torch path, as before"""
    from model import aggregators as A
    g, a = golden, golden_agg
    at, mp = _load(A.AttentionAggregator(8), g, "g4_at_"), _load(A.MaxPoolingAggregator(8, 6), g, "g4_mp_")
    f = torch.from_numpy(g["g4_features"])
    with torch.no_grad():
        np.testing.assert_allclose(at(f, G4_NBRS).numpy(), g["g4_attention"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(mp(f, G4_NBRS).numpy(), g["g4_maxpool"], rtol=1e-5, atol=1e-6)
    at, mp = _load(A.AttentionAggregator(64), a, "at_"), _load(A.MaxPoolingAggregator(64, 48), a, "mp_")
    f, sf, nb = torch.from_numpy(a["features"]), torch.from_numpy(a["self_features"]), _golden_lists(a)
    with torch.no_grad():
        np.testing.assert_allclose(at(f, nb, sf).numpy(), a["attention"], rtol=ac.RTOL, atol=ac.ATOL)
        np.testing.assert_allclose(mp(f, nb).numpy(), a["maxpool"], rtol=ac.RTOL, atol=ac.ATOL)
    # training keeps the tape, on any device
    out = at(f.requires_grad_(True), nb, sf)
    out.sum().backward()
    assert f.grad is not None and at.attention[0].weight.grad is not None
    with pytest.raises(IndexError):
        at(f.detach(), [[96]])
    with pytest.raises(IndexError):
        mp(f.detach(), [[-97]])


def test_entry_points_check_their_arguments():
    """PS_EINVAL for a null pointer or a non-positive H / Hd / T, PS_OK for B == 0 -- decided before anything touches a device"""
    from pinsage_hip import native as nv
    lib = nv.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    aw, gm = lib.ps_attention_weights, lib.ps_gather_max
    assert aw(p, p, 4, 4, p, p, p, 0, 2, p, null) == nv.PS_OK and gm(p, 4, 4, p, p, 0, 2, p, null) == nv.PS_OK
    # an empty batch's tensors have a NULL base: B == 0 is decided before the pointers are looked at
    assert aw(null, p, 4, 4, p, null, null, 0, 2, null, null) == nv.PS_OK and gm(p, 4, 4, null, null, 0, 2, null, null) == nv.PS_OK
    assert aw(null, null, 0, 4, null, null, null, 0, 1, null, null) == nv.PS_OK and gm(null, 0, 4, null, null, 0, 1, null, null) == nv.PS_OK
    assert aw(null, p, 4, 0, p, null, null, 0, 2, null, null) == nv.PS_EINVAL and gm(p, 4, 4, null, null, 0, 0, null, null) == nv.PS_EINVAL
    for k in (0, 1, 4, 5, 6, 9):
        args = [p, p, 4, 4, p, p, p, 1, 2, p, null]
        args[k] = null
        assert aw(*args) == nv.PS_EINVAL, k
    for k in (0, 3, 4, 7):
        args = [p, 4, 4, p, p, 1, 2, p, null]
        args[k] = null
        assert gm(*args) == nv.PS_EINVAL, k
    for hd, t in ((0, 2), (-1, 2), (4, 0), (4, -3)):
        assert aw(p, p, 4, hd, p, p, p, 1, t, p, null) == nv.PS_EINVAL and gm(p, 4, hd, p, p, 1, t, p, null) == nv.PS_EINVAL
    assert aw(p, p, 4, 4, p, p, p, -1, 2, p, null) == nv.PS_EINVAL and gm(p, 4, 4, p, p, -1, 2, p, null) == nv.PS_EINVAL


# ---- GATE_CASES: the launcher gates of csrc/neigh_agg.hip that CASES leaves out -----------------------------------------------
GATE_IDS = [f"g{gi}-B{c[0]}-N{c[1]}-C{c[2]}-T{c[3]}" + ("-offset" if c[4] else "") for gi, c in enumerate(ac.GATE_CASES)]


def test_gate_table_is_the_issues_and_reaches_what_the_old_table_does_not():
    assert [c[:5] for c in ac.GATE_CASES] == [(9, 40, 65, 3, 0), (9, 40, 130, 5, 0), (6, 40, 256, 4, 1), (5, 90, 8, 65, 0),
                                              (5, 200, 8, 130, 0), (5, 200, 6, 130, 0)]
    assert len({c[:5] for c in ac.GATE_CASES}) == len(ac.GATE_CASES) and all(c[5] for c in ac.GATE_CASES)
    old = []
    for ci, (B, N, C, T, _) in enumerate(ac.CASES):
        c = ac.case(ci)
        old.append((ac.agg_facts(B, N, C, T, int(ci == ac.OFFSET_CASE)), ac.plants(c["raw_ids"], c["nvalid"], N)))
    new = {}
    for gi, g in enumerate(ac.GATE_CASES):
        c = ac.gate_case(gi)
        new[GATE_IDS[gi]] = (ac.agg_facts(c["B"], g[1], g[2], g[3], g[4]), ac.plants(c["raw_ids"], c["nvalid"], g[1]))
    for gate, reached in ac.AGG_GATES.items():
        assert not any(reached(f, p) for f, p in old), gate
        rows = [n for n, (f, p) in new.items() if reached(f, p)]
        print(f"{gate}: {rows}")
        assert rows, gate
    f = [new[n][0] for n in GATE_IDS]
    assert [(x["vec"], x["sweeps"]) for x in f[:3]] == [(1, 2), (1, 3), (1, 4)] and 65 - 64 == 1
    assert ac.agg_facts(*ac.GATE_CASES[2][:4])["vec"] == 4                                   # scalar from the alignment alone
    assert [(x["vec"], x["slot_blocks"]) for x in f[3:]] == [(4, 2), (4, 3), (1, 3)] and 65 - 64 == 1
    assert all(p["over"] and p["negative"] for _, p in new.values())
    assert [p["late"] for _, p in new.values()] == [False, False, False, True, True, True]
    assert max(x["slot_blocks"] for x, _ in old) == 2 and max(x["sweeps"] for x, _ in old if x["vec"] == 1) == 1


@pytest.mark.parametrize("gi", range(len(ac.GATE_CASES)), ids=GATE_IDS)
def test_gate_case_plants_what_it_says(gi):
    c = ac.gate_case(gi)
    N, T, r = c["N"], c["T"], c["rows"]
    ids, nv = c["raw_ids"], c["nvalid"]
    keep = ac.kept(ids, nv, N)
    assert c["B"] >= ac.GATE_CASES[gi][0] and sorted(r.values()) == list(range(c["B"] - 7, c["B"]))
    assert [int(nv[r[k]]) for k in ("over", "huge", "twin", "neg", "negmin")] == [T + 5, 2 ** 31 - 1, T, -1, -2 ** 31]
    assert np.array_equal(ids[r["over"]], ids[r["twin"]]) and np.array_equal(ids[r["huge"]], ids[r["twin"]])
    assert np.array_equal(c["u"][r["over"]], c["u"][r["twin"]]) and np.array_equal(c["u"][r["huge"]], c["u"][r["twin"]])
    assert np.array_equal(keep[r["over"]], keep[r["twin"]]) and np.array_equal(keep[r["huge"]], keep[r["twin"]])
    assert keep[r["twin"]].sum() == (T - 1 if T >= 3 else T)
    assert not keep[r["neg"]].any() and not keep[r["negmin"]].any() and ((ids[r["neg"]] >= 0) & (ids[r["neg"]] < N)).all()
    if T > 64:
        assert not keep[r["late"], :64].any() and keep[r["late"], 64:].all()
        assert {-1, N, 2 ** 31 - 1} == set(ids[r["late"], :64].tolist())
    one = ids[r["one"]][keep[r["one"]]]
    assert len(set(one.tolist())) == 1 and one.size == (T - 1 if T >= 3 else T)
    assert keep[0].all() and {-1, N, 2 ** 31 - 1} <= set(ids.ravel().tolist())


@pytest.mark.parametrize("gi", range(len(ac.GATE_CASES)), ids=GATE_IDS)
def test_exact_scores_and_their_softmax(gi):
    """the softmax of the exact fp32 scores lies inside the tolerance the fp64 reference is held to
    (tests/test_hip_aggregators.py::test_attention_weights), clamped rows equal their twin, a row whose kept slots all name one
    neighbour has reference weights of exactly 1 / n, and the derived bound is far below that tolerance"""
    c = ac.gate_case(gi)
    r = c["rows"]
    s = ac.attention_scores_exact(c["u"], c["v"], c["w2"], c["raw_ids"], c["nvalid"], c["vec"])
    keep = ac.kept(c["raw_ids"], c["nvalid"], c["N"])
    assert s.dtype == np.float32 and np.array_equal(np.isfinite(s), keep) and np.isneginf(s[~keep]).all()
    a = ac.softmax_of_scores(s)
    ref = ac.attention_weights_ref(c["u"], c["v"], c["w2"], c["raw_ids"], c["nvalid"])
    np.testing.assert_allclose(a, ref, rtol=ac.RTOL, atol=ac.ATOL)
    assert np.array_equal(s[r["over"]], s[r["twin"]]) and np.array_equal(s[r["huge"]], s[r["twin"]])
    n = int(keep[r["one"]].sum())
    assert len(set(s[r["one"]][keep[r["one"]]].tolist())) == 1                                 # equal scores, bit for bit
    assert (a[r["one"]][keep[r["one"]]] == 1.0 / n).all() and (ref[r["one"]][keep[r["one"]]] == 1.0 / n).all()
    b = ac.attention_bound(s, c["T"])
    assert b.shape == a.shape and not b[~keep].any() and (b[keep] > 0).all()
    assert (b[keep] <= 1e-5 * a[keep] + 2.0 ** -149).all()                                     # at least ten times tighter than RTOL alone
    print(f"gate {gi}: bound / weight between {np.min(b[keep] / a[keep]):.2e} and {np.max(b[keep] / a[keep]):.2e}")


def test_cases_tell_the_scores_from_a_near_miss():
    """a sequential instead of a tree wave sum; and the other path's lane assignment (vec 4 for 1, 1 for 4)"""
    seq, lanes = [], []
    for gi, g in enumerate(ac.GATE_CASES):
        c = ac.gate_case(gi)
        args = (c["u"], c["v"], c["w2"], c["raw_ids"], c["nvalid"])
        s = ac.attention_scores_exact(*args, c["vec"])
        if not np.array_equal(ac.attention_scores_exact(*args, c["vec"], sequential=True), s):
            seq.append(GATE_IDS[gi])
        if g[2] % 4 == 0 and not np.array_equal(ac.attention_scores_exact(*args, 5 - c["vec"]), s):
            lanes.append(GATE_IDS[gi])
    print("sequential wave sum differs on", seq, "; the other path's lanes on", lanes)
    assert seq and lanes
