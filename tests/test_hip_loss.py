"""model.loss drop-in and the kernels behind it (ps_hardest_negative = the GEMM with the row-arg-max epilogue, ps_margin_loss,
ps_margin_loss_bwd).

  * CPU only: the module imports from the drop-in tree with the reference's signatures, the classes on CPU tensors against the
    reference's outputs (tests/golden/reference_golden_loss.npz, tests/golden/make_golden_loss.py), the C entries reject invalid
    arguments before touching a device;
  * kernel vs slab, exact: maximum bit for bit and the smallest index of each row's maximum against torch on a dense.linear
    slab (the config shape, D = 256, unaligned, one row, one candidate, 59 047 candidates, a tie-heavy matrix, the diagonal
    left out), the per-query form bit-equal to the shared form on equal data;
  * losses against the reference's within 4 (D + 2) 2^-24 max|q| max|x| (two similarities per row, each side within
    (D + 2) 2^-24 |q||x| of exact), arg-max and active mask equal;
  * gradients equal to the closed form evaluated in float64 over the fixture's indices and mask, and to the reference's stored
    gradients (equal as numbers: a zero matches a zero of either sign).  For a batch size that is no power of two g = 1 / B
    rounds: within 2 ulp of the reference wherever an entry is a single product or the two-term dQ, the same zeros, and within
    one ulp of the terms' magnitude sum per term of the float64 closed form.  (Measured on an MI355X, B = 48: dQ / dP / per-query
    dX 0 ulp from the reference; entries that sum over query rows -- shared dX, batch-hard dP -- up to 128 ulp of a cancelled
    result from the reference, which sums in its own order, at 0.25 of that tolerance: an ulp of the result is no yardstick
    for a sum that cancels.)
  * no [B, N] / [B, N, D] tensor in either direction (peak memory), launch counts, and one training step of PinSage.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from loss_cases import _closed_form, _closed_form_magnitude  # noqa: E402  (the fp64 closed form: shared with tests/test_loss_cases.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_golden_loss.npz")
FORMS = ("shared", "perq", "twod", "bh")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _f16(gold, key, rows, cols):
    """a float16 matrix stored as [2, n] byte planes (low bytes, high bytes) -> float32"""
    planes = gold[key]
    return np.ascontiguousarray(planes.T).view("<f2").reshape(rows, cols).astype(np.float32)


def _case(gold, name):
    B, N, D = [int(v) for v in gold[f"{name}_shape"]]
    Q, P, X = _f16(gold, f"{name}_Q16", B, D), _f16(gold, f"{name}_P16", B, D), _f16(gold, f"{name}_X16", N, D)
    return B, N, D, Q, P, X, gold[f"{name}_hidx"].astype(np.int64)


def _bound(D, Q, *others):
    nq = float(np.linalg.norm(Q.astype(np.float64), axis=-1).max())
    nx = max(float(np.linalg.norm(o.astype(np.float64), axis=-1).max()) for o in others)
    return 4 * (D + 2) * 2.0 ** -24 * nq * nx


def _run_form(ml, form, Q, P, X, hidx, dev, margin, scale=None):
    """one forward (+ backward) of a drop-in class -> (loss, (dQ, dP, dX) or None); shared: X is a leaf [N, D] passed expanded"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True)       # noqa: E731
    q, p = t(Q), t(P)
    x = None
    if form == "bh":
        loss = ml.BatchHardTripletLoss(margin)(q, p)
    else:
        x = t(X if form == "shared" else X[hidx] if form == "perq" else X[hidx[:, 0]])
        neg = x.unsqueeze(0).expand(Q.shape[0], -1, -1) if form == "shared" else x
        loss = ml.MaxMarginRankingLoss(margin)(q, p, neg)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad and loss.device.type == dev.type
    (loss if scale is None else loss * scale).backward()
    grads = tuple(None if v is None else v.grad.detach().cpu().numpy() for v in (q, p, x))
    return float(loss.detach()), grads


def _form_input(form, X, hidx):
    return None if form == "bh" else X if form == "shared" else X[hidx] if form == "perq" else X[hidx[:, 0]]


# ---------------------------------------------------------------------------------------------------------- CPU only

def test_loss_modules_import_with_the_reference_signatures(gold):
    import model.loss as ml
    import data.negative_sampler as ns
    pkg = os.path.join(ROOT, "movie-recommendation-engine_amd")
    assert os.path.realpath(ml.__file__).startswith(pkg) and os.path.realpath(ns.__file__).startswith(pkg)
    for key in gold.files:
        if key.startswith("sig_"):
            cls, meth = key[4:].split(".")
            owner = ns if cls == "NegativeSampler" else ml
            assert str(inspect.signature(getattr(getattr(owner, cls), meth))) == str(gold[key]), key
    cl = ml.CurriculumLoss()
    assert (cl.margin, cl.epoch, cl.max_epochs, cl.hard_negative_factor) == (0.1, 0, 10, 2.0)
    assert isinstance(cl.base_loss, ml.MaxMarginRankingLoss) and cl.base_loss.margin == 0.1
    cl.update_epoch(4)
    assert cl.epoch == 4 and ml.BatchHardTripletLoss().margin == 0.1


@pytest.mark.parametrize("name", ["cfg", "una", "sm", "np2"])
def test_cpu_tensors_match_the_reference(gold, name):
    import model.loss as ml
    B, N, D, Q, P, X, hidx = _case(gold, name)
    margin = float(gold["margin"])
    cpu = torch.device("cpu")
    for form in FORMS:
        loss, grads = _run_form(ml, form, Q, P, X, hidx, cpu, margin)
        ref = float(gold[f"{name}_{form}_loss"])
        print(f"{name} {form}: loss {loss:.9f} reference {ref:.9f} bound {_bound(D, Q, X, P):.3e}")
        assert abs(loss - ref) <= _bound(D, Q, X, P), (name, form)
        idx, active = gold[f"{name}_{form}_idx"].astype(np.int64), gold[f"{name}_{form}_active"]
        cf = _closed_form(Q, P, _form_input(form, X, hidx), idx, active, form)
        for got, want in zip(grads, cf):
            if want is not None:
                assert np.array_equal(got != 0, want != 0), (name, form)       # arg-max / active pattern
    for e in [int(v) for v in gold["epochs"]]:
        t = lambda a: torch.from_numpy(a)       # noqa: E731
        cl = ml.CurriculumLoss(margin, epoch=e)
        loss = cl(t(Q), t(P), t(X).unsqueeze(0).expand(B, -1, -1), t(X[hidx]))
        assert abs(float(loss) - float(gold[f"{name}_cur_{e}_loss"])) <= 3 * _bound(D, Q, X, P), (name, e)


def test_cpu_edge_cases_follow_the_reference():
    import model.loss as ml
    q = torch.zeros(0, 8)
    assert torch.isnan(ml.MaxMarginRankingLoss()(q, q, q))                                   # mean of nothing
    with pytest.raises((RuntimeError, IndexError)):
        ml.BatchHardTripletLoss()(q, q)                                                       # max over an empty dimension
    with pytest.raises((RuntimeError, IndexError)):
        ml.MaxMarginRankingLoss()(torch.ones(3, 8), torch.ones(3, 8), torch.ones(3, 0, 8))   # max over no candidate
    h = ml.MaxMarginRankingLoss()(torch.ones(2, 4).half(), torch.ones(2, 4).half(), torch.ones(2, 3, 4).half())
    assert h.dtype == torch.float16


def test_loss_entries_reject_invalid_arguments():
    from pinsage_hip import native
    if not native.have_lib():
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(native.SO_PATH)
    i64, i32, p, f32 = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    one = p(16)       # never dereferenced: every call below returns before any device work
    hn = lambda *a: lib.ps_hardest_negative(*a)                                              # noqa: E731
    assert hn(one, i64(-1), i32(8), one, i64(4), i32(0), one, one, one, p(0)) == native.PS_EINVAL
    assert hn(one, i64(4), i32(0), one, i64(4), i32(0), one, one, one, p(0)) == native.PS_EINVAL
    assert hn(one, i64(4), i32(8), one, i64(-4), i32(0), one, one, one, p(0)) == native.PS_EINVAL
    assert hn(one, i64(4), i32(8), one, i64(0), i32(0), one, one, one, p(0)) == native.PS_EINVAL      # no candidate
    assert hn(p(0), i64(4), i32(8), one, i64(4), i32(0), one, one, one, p(0)) == native.PS_EINVAL
    assert hn(one, i64(4), i32(8), p(0), i64(4), i32(0), one, one, one, p(0)) == native.PS_EINVAL
    assert hn(one, i64(4), i32(8), one, i64(4), i32(0), p(0), one, one, p(0)) == native.PS_EINVAL
    assert hn(one, i64(4), i32(8), one, i64(4), i32(0), p(20), one, one, p(0)) == native.PS_EINVAL    # best not 8-B aligned
    assert hn(one, i64(4), i32(8), one, i64(4), i32(8), one, one, one, p(0)) == native.PS_EINVAL      # unknown flag
    assert hn(one, i64(4), i32(8), one, i64(4), i32(3), one, one, one, p(0)) == native.PS_EINVAL      # per-query + diagonal
    assert hn(one, i64(1 << 31), i32(8), one, i64(4), i32(0), one, one, one, p(0)) == native.PS_EUNSUPPORTED
    assert hn(one, i64(4), i32(8), one, i64(1 << 31), i32(0), one, one, one, p(0)) == native.PS_EUNSUPPORTED
    assert hn(p(0), i64(0), i32(8), p(0), i64(4), i32(0), p(0), p(0), p(0), p(0)) == native.PS_OK
    ml_ = lambda *a: lib.ps_margin_loss(*a)                                                  # noqa: E731
    assert ml_(one, one, i64(-1), i32(8), one, f32(0.1), one, one, one, one, p(0)) == native.PS_EINVAL
    assert ml_(one, one, i64(4), i32(0), one, f32(0.1), one, one, one, one, p(0)) == native.PS_EINVAL
    assert ml_(one, p(0), i64(4), i32(8), one, f32(0.1), one, one, one, one, p(0)) == native.PS_EINVAL
    assert ml_(one, one, i64(4), i32(8), one, f32(0.1), one, one, one, p(0), p(0)) == native.PS_EINVAL
    assert ml_(one, one, i64(1 << 31), i32(8), one, f32(0.1), one, one, one, one, p(0)) == native.PS_EUNSUPPORTED
    assert ml_(p(0), p(0), i64(0), i32(8), p(0), f32(0.1), p(0), p(0), p(0), p(0), p(0)) == native.PS_OK
    bw = lambda *a: lib.ps_margin_loss_bwd(*a)                                               # noqa: E731
    assert bw(one, one, one, i64(-1), i64(4), i32(8), i32(0), one, one, one, one, one, one, p(0)) == native.PS_EINVAL
    assert bw(one, one, one, i64(4), i64(4), i32(0), i32(0), one, one, one, one, one, one, p(0)) == native.PS_EINVAL
    assert bw(one, one, one, i64(4), i64(4), i32(8), i32(7), one, one, one, one, one, one, p(0)) == native.PS_EINVAL
    assert bw(one, one, one, i64(4), i64(4), i32(8), i32(0), p(0), one, one, one, one, one, p(0)) == native.PS_EINVAL
    assert bw(one, one, one, i64(4), i64(4), i32(8), i32(0), one, one, p(0), one, one, one, p(0)) == native.PS_EINVAL
    assert bw(one, one, p(0), i64(4), i64(4), i32(8), i32(0), one, one, one, one, one, one, p(0)) == native.PS_EINVAL
    assert bw(one, one, p(0), i64(4), i64(5), i32(8), i32(2), one, one, one, one, one, p(0), p(0)) == native.PS_EINVAL  # N != B
    assert bw(one, one, one, i64(1 << 31), i64(4), i32(8), i32(0), one, one, one, one, one, one, p(0)) == native.PS_EUNSUPPORTED
    assert bw(p(0), p(0), p(0), i64(0), i64(4), i32(8), i32(0), p(0), p(0), p(0), p(0), p(0), p(0), p(0)) == native.PS_OK
    assert lib.ps_abi_version() == 1


# ---------------------------------------------------------------------------------------------------------- GPU

def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _unit(n, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(_dev()).contiguous()


def _tie_heavy(N, D, seed):
    """values on five levels, duplicated rows, all-zero rows, a -0.0 row: many exact ties (as in tests/test_hip_evaluation.py)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = (torch.randint(-2, 3, (N, D), generator=g).float() * 0.5)
    X[100:200] = X[0:100]
    X[300:340] = 0.0
    X[341] = -0.0
    X[N - 50:] = X[10:60]
    return X.to(_dev()).contiguous()


def _slab_argmax(S):
    """(row maximum, smallest index attaining it) of a slab, with torch ops only"""
    m = S.max(dim=1).values
    cols = torch.arange(S.size(1), device=S.device).expand_as(S)
    first = torch.where(S == m[:, None], cols, torch.full_like(cols, S.size(1))).min(dim=1).values
    return m, first


SLAB_CASES = [
    # name, B, N, D, data
    ("config", 512, 500, 128, "unit"),
    ("d256", 2048, 500, 256, "unit"),
    ("unaligned", 64, 37, 100, "unit"),
    ("one_row", 1, 500, 128, "unit"),
    ("one_candidate", 77, 1, 64, "unit"),
    ("catalogue", 512, 59047, 128, "unit"),
    ("ties", 700, 4099, 64, "ties"),
    ("ties_unaligned", 300, 2053, 36, "ties"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,N,D,data", SLAB_CASES, ids=[c[0] for c in SLAB_CASES])
def test_hardest_negative_equals_the_slab(name, B, N, D, data):
    from pinsage_hip import dense, loss as hl
    if data == "ties":
        X = _tie_heavy(N, D, 5)
        Q = X[torch.randperm(N, generator=torch.Generator().manual_seed(6))[:B].to(X.device)].contiguous()
        Q[: B // 2, 4:] = 0.0          # four live columns on five levels: a few hundred distinct similarities, so the maximum is shared
    else:
        Q, X = _unit(B, D, 1), _unit(N, D, 2)
    S = dense.linear(Q, X)
    want, first = _slab_argmax(S)
    sim, idx = hl.hardest_negative(Q, X)
    assert sim.dtype == torch.float32 and idx.dtype == torch.int64 and sim.shape == idx.shape == (B,)
    assert torch.equal(sim.view(torch.int32), want.view(torch.int32)), name
    assert torch.equal(idx, first), name
    if data == "ties":
        tied = ((S == want[:, None]).sum(dim=1) > 1).float().mean().item()
        assert tied > 0.25, f"{name}: only {tied:.2f} of the rows have a tied maximum"
    # the per-query form on the same data
    if B * N * D <= 1 << 25:
        sim3, idx3 = hl.hardest_negative(Q, X.unsqueeze(0).expand(B, -1, -1).contiguous())
        assert torch.equal(sim3.view(torch.int32), sim.view(torch.int32)) and torch.equal(idx3, idx), name


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,data", [(512, 128, "unit"), (200, 100, "unit"), (1, 32, "unit"), (700, 64, "ties")])
def test_hardest_negative_without_the_diagonal(B, D, data):
    from pinsage_hip import dense, loss as hl
    Q = _unit(B, D, 3)
    P = _tie_heavy(B, D, 7) if data == "ties" else _unit(B, D, 4)
    if data == "ties":
        Q = P.roll(3, 0).contiguous()
    S = dense.linear(Q, P)
    S[torch.arange(B), torch.arange(B)] = float("-inf")
    want, first = _slab_argmax(S)
    sim, idx = hl.hardest_negative(Q, P, exclude_diag=True)
    assert torch.equal(sim.view(torch.int32), want.view(torch.int32))
    if B == 1:
        assert idx.item() == -1 and sim.item() == float("-inf")
    else:
        assert torch.equal(idx, first)


@pytest.mark.gpu
def test_a_nan_similarity_is_the_row_maximum():
    from pinsage_hip import loss as hl
    Q, X = _unit(70, 64, 8), _unit(300, 64, 9)
    X[17, 3] = float("nan")
    X[250, 0] = float("nan")
    sim, idx = hl.hardest_negative(Q, X)
    assert torch.isnan(sim).all() and (idx == 17).all()    # the first NaN, as torch.max


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg", "una", "sm", "np2"])
def test_losses_match_the_reference(gold, name):
    import model.loss as ml
    from pinsage_hip import loss as hl
    B, N, D, Q, P, X, hidx = _case(gold, name)
    margin, dev = float(gold["margin"]), _dev()
    bound = _bound(D, Q, X, P)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    modes = {"shared": hl.SHARED, "perq": hl.PER_QUERY, "twod": hl.PER_QUERY, "bh": hl.BATCH_HARD}
    for form in FORMS:
        loss, _ = _run_form(ml, form, Q, P, X, hidx, dev, margin)
        ref = float(gold[f"{name}_{form}_loss"])
        print(f"{name} {form}: loss {loss:.9f} reference {ref:.9f} |diff| {abs(loss - ref):.3e} bound {bound:.3e}")
        assert abs(loss - ref) <= bound, (name, form)
        xin = _form_input(form, X, hidx)
        if form == "twod":
            xin = xin[:, None, :]
        _, idx, active = hl.forward_state(t(Q), t(P), None if xin is None else t(xin), modes[form], margin)
        assert np.array_equal(idx.cpu().numpy(), gold[f"{name}_{form}_idx"].astype(np.int64)), (name, form)
        assert np.array_equal(active.cpu().numpy(), gold[f"{name}_{form}_active"]), (name, form)
    for e in [int(v) for v in gold["epochs"]]:
        cl = ml.CurriculumLoss(margin, epoch=e)
        q = t(Q).requires_grad_(True)
        loss = cl(q, t(P), t(X).unsqueeze(0).expand(B, -1, -1), t(X[hidx]))
        assert loss.dim() == 0 and loss.is_cuda and loss.requires_grad and loss.dtype == torch.float32
        w = min(e, 10) / 10 * 2.0 if e >= 1 else 0.0
        assert abs(float(loss.detach()) - float(gold[f"{name}_cur_{e}_loss"])) <= (1 + w) * bound, (name, e)
        if e == 3:
            nohard = cl(q, t(P), t(X).unsqueeze(0).expand(B, -1, -1))
            assert abs(float(nohard.detach()) - float(gold[f"{name}_cur_nohard_loss"])) <= bound, name


def _ulp_diff(a, b):
    """distance in float32 steps between two float32 arrays (as numbers: -0.0 == +0.0)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg", "una", "sm", "np2"])
@pytest.mark.parametrize("scale", [None, 3.0])
def test_gradients_equal_the_closed_form(gold, name, scale):
    import model.loss as ml
    B, N, D, Q, P, X, hidx = _case(gold, name)
    margin, dev = float(gold["margin"]), _dev()
    pow2 = B & (B - 1) == 0
    for form in FORMS:
        _, grads = _run_form(ml, form, Q, P, X, hidx, dev, margin, scale)
        _, again = _run_form(ml, form, Q, P, X, hidx, dev, margin, scale)
        idx, active = gold[f"{name}_{form}_idx"].astype(np.int64), gold[f"{name}_{form}_active"]
        xin = _form_input(form, X, hidx)
        cf = _closed_form(Q, P, xin, idx, active, form, 1.0 if scale is None else scale)
        mag = _closed_form_magnitude(Q, P, xin, idx, active, form, 1.0 if scale is None else scale)
        for which, got, rerun, want in zip(("dQ", "dP", "dX"), grads, again, cf):
            if want is None:
                assert got is None
                continue
            assert got.shape == want.shape and got.dtype == np.float32, (name, form, which)
            assert np.array_equal(got.view(np.int32), rerun.view(np.int32)), (name, form, which, "two runs differ")
            if pow2:      # g = 1 / B is a power of two, the inputs are float16 values: every entry is exact in fp32
                assert np.array_equal(got, want.astype(np.float32)), (name, form, which)
            else:
                # g = 1 / B is rounded, so is every product g * v and every sum: n products, n - 1 sums and g itself are 2 n roundings
                # of at most half an ulp of the entry's magnitude sum |g v_1| + ... + |g v_n| (an ulp of the RESULT means nothing
                # where the terms cancel: dQ = g x - g p with x close to p).  n = 2 for dQ, 1 for dP and the per-query dX.
                msum, terms = mag[which]
                err = np.abs(got.astype(np.float64) - want)
                tol = np.maximum(terms, 1) * np.spacing(msum.astype(np.float32)).astype(np.float64)
                print(f"{name} {form} {which}: max error / tolerance {float((err / tol).max()):.3f}")
                assert (err <= tol).all(), (name, form, which)
                assert np.array_equal(got == 0, want == 0), (name, form, which)
            key = f"{name}_{form}_{which}"
            if scale is None and key in gold.files:      # the reference's own autograd gradients (small cases)
                ref = gold[key]
                if pow2:
                    assert np.array_equal(got, ref), key
                else:
                    # within 2 ulp of the reference wherever an entry is one product, or the two-term dQ.  An entry that SUMS over
                    # several query rows (shared dX, batch-hard dP) is summed by the reference in its own order, not in ascending
                    # b: two correct fp32 sums of the same terms differ by up to an ulp of the terms' magnitude per rounding on
                    # either side, which is many ulps of a result that cancelled (measured: np2 shared dX, 64 ulp of an entry of
                    # 1e-5 summed from terms of 1e-2, 0.3 of the tolerance below)
                    summed = (form == "shared" and which == "dX") or (form == "bh" and which == "dP")
                    few = mag[which][1] <= (1 if summed else 2)
                    assert _ulp_diff(got, ref)[few].max() <= 2 and np.array_equal(got == 0, ref == 0), key
                    err_ref = np.abs(got.astype(np.float64) - ref.astype(np.float64))
                    print(f"{key}: max error / tolerance vs the reference {float((err_ref / (2 * tol)).max()):.3f}, "
                          f"max ulp distance {int(_ulp_diff(got, ref).max())}")
                    assert (err_ref <= 2 * tol).all(), key


@pytest.mark.gpu
def test_curriculum_gradients_match_the_reference(gold):
    import model.loss as ml
    name = "sm"
    B, N, D, Q, P, X, hidx = _case(gold, name)
    dev = _dev()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True)       # noqa: E731
    q, p, xs, xh = t(Q), t(P), t(X), t(X[hidx])
    ml.CurriculumLoss(float(gold["margin"]), epoch=3)(q, p, xs.unsqueeze(0).expand(B, -1, -1), xh).backward()
    assert xs.grad.shape == (N, D)
    # dQ sums four products (g x and g p of the base and of the 0.6-weighted hard loss), dXs up to B of them; the weight is no
    # power of two, so products and sums round: each term is below 2 / B in magnitude, so every rounding is at most half an ulp
    # of 2 / B, and the reference rounds as often in its own order -- one ulp of 2 / B per term covers both sides
    ulp = float(np.spacing(np.float32(2.0 / B)))
    assert np.abs(q.grad.cpu().numpy().astype(np.float64) - gold["sm_cur_3_dQ"]).max() <= 4 * ulp
    hits = np.bincount(gold["sm_shared_idx"].astype(np.int64), minlength=N).max()
    assert np.abs(xs.grad.cpu().numpy().astype(np.float64) - gold["sm_cur_3_dXs"]).max() <= (hits + 1) * ulp


@pytest.mark.gpu
def test_double_backward_raises():
    import model.loss as ml
    q = _unit(32, 16, 1).requires_grad_(True)
    loss = ml.BatchHardTripletLoss()(q, _unit(32, 16, 2))
    (g,) = torch.autograd.grad(loss, q, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.gpu
def test_shared_form_writes_no_slab_and_few_launches():
    import model.loss as ml
    from pinsage_hip import native as nv
    B, N, D = 2048, 500, 256
    q, p, x = (_unit(n, D, s).requires_grad_(True) for n, s in ((B, 1), (B, 2), (N, 3)))
    crit = ml.MaxMarginRankingLoss(0.1)
    crit(q, p, x.unsqueeze(0).expand(B, -1, -1)).backward()          # warm-up: library handles, allocator pools
    q.grad = p.grad = x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = crit(q, p, x.unsqueeze(0).expand(B, -1, -1))
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    grads = 4 * (2 * B * D + N * D)
    print(f"peak rise {rise} bytes, gradients {grads} bytes, the [B, N, D] product would be {4 * B * N * D} bytes")
    assert x.grad.shape == (N, D) and q.grad.shape == (B, D) and p.grad.shape == (B, D)
    assert rise <= grads + (1 << 20)

    q.grad = p.grad = x.grad = None
    timer = nv.KernelTimer()
    nv.set_timer(timer)
    try:
        loss = crit(q, p, x.unsqueeze(0).expand(B, -1, -1))
        fwd = {k: v["launches"] for k, v in timer.summary().items()}
        timer.events.clear()
        loss.backward()
        bwd = {k: v["launches"] for k, v in timer.summary().items()}
    finally:
        nv.set_timer(None)
    assert sum(fwd.values()) <= 3 and "ps_linear" not in fwd and fwd.get("ps_hardest_negative") == 1, fwd
    assert sum(bwd.values()) <= 2 and "ps_linear" not in bwd, bwd


@pytest.mark.gpu
def test_a_view_without_a_base_takes_the_per_query_path(gold):
    """the same numbers whichever path the negatives take: an expanded view, its materialised copy, a non-leaf base"""
    import model.loss as ml
    B, N, D, Q, P, X, hidx = _case(gold, "una")
    dev = _dev()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    crit = ml.MaxMarginRankingLoss(0.1)
    q, p = t(Q), t(P)
    x1 = t(X).requires_grad_(True)
    l1 = crit(q, p, x1.unsqueeze(0).expand(B, -1, -1))
    l1.backward()
    x2 = t(X).requires_grad_(True)
    l2 = crit(q, p, x2.unsqueeze(0).expand(B, -1, -1).contiguous())
    l2.backward()
    table = torch.cat([t(X), t(X)]).requires_grad_(True)
    l3 = crit(q, p, table[N:].unsqueeze(0).expand(B, -1, -1))       # the base is the [2 N, D] table: a strided alias
    l3.backward()
    assert torch.equal(l1, l2) and torch.equal(l1, l3)
    assert torch.equal(x1.grad, x2.grad) and torch.equal(table.grad[N:], x1.grad) and not table.grad[:N].any()


@pytest.mark.gpu
def test_one_training_step_of_pinsage():
    import model.loss as ml
    from model.pinsage import PinSage
    from pinsage_hip import synth
    from utils.random_walk import RandomWalkSampler
    dev = _dev()
    M = 400
    ei, ew = synth.bipartite_ratings(300, M, 12000, seed=1)
    sampler = RandomWalkSampler(ei, ew, walk_length=2, num_walks=100, device=dev)
    torch.manual_seed(0)
    model = PinSage(32, 64, 32, num_layers=2).to(dev).train()
    x = torch.randn(M, 32).to(dev)
    g = torch.Generator().manual_seed(1)
    qi, pi, ni = (torch.randint(0, M, (n,), generator=g).to(dev) for n in (128, 128, 50))
    crit = ml.MaxMarginRankingLoss(0.1)

    def losses():
        np.random.seed(42)                                         # the same neighbour samples on every call
        emb = model.get_embeddings(x, sampler, num_neighbors=10)
        assert emb.requires_grad
        neg = emb[ni].unsqueeze(0).expand(qi.numel(), -1, -1)
        return crit(emb[qi], emb[pi], neg), ml.torch_max_margin(emb[qi], emb[pi], neg, 0.1)

    params = [w for w in model.parameters() if w.requires_grad]
    ours, plain = losses()
    assert abs(float(ours) - float(plain)) <= 4 * 34 * 2.0 ** -24
    assert float(ours) > 0
    g_ours = torch.autograd.grad(ours, params, retain_graph=True, allow_unused=True)
    g_plain = torch.autograd.grad(plain, params, allow_unused=True)
    seen = 0
    for a, b in zip(g_ours, g_plain):
        assert (a is None) == (b is None)
        if a is not None:
            seen += 1
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    assert seen >= 6
    opt = torch.optim.Adam(params, lr=1e-3)
    opt.zero_grad()
    first, _ = losses()
    first.backward()
    opt.step()
    after, _ = losses()
    print(f"loss {float(first):.6f} -> {float(after):.6f} after one Adam step")
    assert float(after) < float(first)
