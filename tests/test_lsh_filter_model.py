"""The arithmetic of the staged LSH encode (csrc/lsh_filter.hip), restated in numpy: the round-to-nearest-even split of an fp32
into bf16 hi + lo, the three-product estimate and the flag rule  |f| > c nx na  (strict; c = 2^-12 max(1, D / 256); nx, na =
row norms inflated by 1 + 2^-10, +inf outside [2^-30, 2^30]).  Two claims are held here, without a GPU:

  * the representation error alone -- the exact value of sum xh ah + xh al + xl ah against the exact sum x a -- stays below
    2^-16 S, S = sum |x_k a_k|  (two splits of relative error 2^-18 each, the dropped xl al term below 2^-18);
  * no dot the rule leaves UNFLAGGED has another sign than the oracle's fp32 fmaf chain, on unit-norm, +-1-valued and heavily
    cancelling rows; the estimate is accumulated in fp32 in MFMA-sized steps of 16 k.
"""
import numpy as np
import pytest

from oracle import pinsage_oracle as orc


def bf16_rne(v):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split(v):
    hi = bf16_rne(v)
    return hi, bf16_rne(v - hi)               # v - hi is exact in fp32


def bound(m):
    """per row: the norm bound of the kernel, +inf where the filter must not be trusted"""
    n = np.sqrt((m.astype(np.float64) ** 2).sum(axis=1))
    return np.where((n >= 2.0 ** -30) & (n <= 2.0 ** 30), n * (1 + 2.0 ** -10), np.inf)


def estimate(x, A):
    """f32 accumulation over k steps of 16, each step's three partial products summed exactly first"""
    xh, xl = (t.astype(np.float64) for t in split(x))
    ah, al = (t.astype(np.float64) for t in split(A))
    f = np.zeros((x.shape[0], A.shape[0]), dtype=np.float32)
    for k in range(0, x.shape[1], 16):
        s = slice(k, k + 16)
        for u, v in ((xh, al), (xl, ah), (xh, ah)):
            f = (f.astype(np.float64) + u[:, s] @ v[:, s].T).astype(np.float32)
    exact = xh @ ah.T + xh @ al.T + xl @ ah.T
    return f, exact


def cases(D):
    rs = np.random.RandomState(1000 + D)
    n, nbits = 96, 2 * D
    unit = rs.standard_normal((n, D)).astype(np.float32)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True).astype(np.float32)
    rot = orc.lsh_rotation_matrix(D, nbits)
    pm_x = rs.choice([-1.0, 1.0], size=(n, D)).astype(np.float32)
    pm_a = rs.choice([-1.0, 1.0], size=(nbits, D)).astype(np.float32)
    # heavily cancelling: pairs (v, -v(1 + e)) of large entries against nearly equal rotation entries
    big = (rs.standard_normal((n, D)) * 1000.0).astype(np.float32)
    big[:, 1::2] = -big[:, 0::2] * (1.0 + rs.standard_normal((n, D // 2)).astype(np.float32) * 1e-3)
    smooth = np.repeat(rs.standard_normal((nbits, D // 2)), 2, axis=1).astype(np.float32)
    smooth += (rs.standard_normal((nbits, D)) * 1e-4).astype(np.float32)
    return {"unit": (unit, rot), "pm1": (pm_x, pm_a), "cancel": (big, smooth)}


@pytest.mark.parametrize("D", [32, 128, 256])
def test_split_estimate_and_flag_rule(D):
    c = 2.0 ** -12 * max(1.0, D / 256.0)
    for name, (x, A) in cases(D).items():
        f, exact = estimate(x, A)
        x64, a64 = x.astype(np.float64), A.astype(np.float64)
        S = np.abs(x64) @ np.abs(a64).T
        rep = np.abs(exact - x64 @ a64.T)
        assert (rep <= 2.0 ** -16 * S).all(), (name, float((rep / S).max()))
        _, chain = orc.lsh_encode(x, A)
        thr = c * bound(x)[:, None] * bound(A)[None, :]
        trusted = np.abs(f.astype(np.float64)) > thr
        assert ((f >= 0) == (chain >= 0))[trusted].all(), name
        # the margin the kernel is held to on the GPU (c / 4): here 2^-16 S of representation, 3 D / 16 roundings of the
        # estimate's accumulator and D of the chain's, 2^-24 S each -- below 2^-14.9 S at D = 256, and S <= |x| |a|
        assert (np.abs(f.astype(np.float64) - chain) <= 0.25 * thr).all(), name
        if name == "unit":
            share = 1.0 - trusted.mean()
            assert 0.0 < share < 0.01, share            # erf(c sqrt(D / 2)): 0.3 % at D = 256
        if name == "pm1":
            assert not trusted[chain == 0].any() and (chain == 0).any()                  # exact zeros are always rechecked


def test_guards():
    """zero, tiny, huge and non-finite rows get an infinite bound: every one of their dots is flagged"""
    x = np.zeros((6, 32), dtype=np.float32)
    x[1] = 2.0 ** -40
    x[2] = 2.0 ** 40
    x[3, 0] = np.nan
    x[4, 0] = np.inf
    x[5] = 1.0
    b = bound(x)
    assert np.isinf(b[:5]).all() and np.isfinite(b[5])
    f = np.float32(0.0)
    assert not (abs(f) > 0.0) and not (np.float32(np.nan) > 0.0)        # f = 0 and NaN fail the strict comparison
    hi, lo = split(np.array([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 3.1415927, -1e-3], dtype=np.float32))
    assert hi[0] == 1.0 and lo[0] == 2.0 ** -8                           # ties go to the even neighbour: down here,
    assert hi[1] == 1.0 + 2.0 ** -6 and lo[1] == -2.0 ** -8              # up here
    v = np.array([3.1415927, -1e-3], dtype=np.float32)
    assert (np.abs(v - hi[2:].astype(np.float64) - lo[2:]) <= 2.0 ** -18 * np.abs(v)).all()
