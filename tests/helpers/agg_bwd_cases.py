"""An exact numpy restatement of the backward kernels of the neighbour gathers (csrc/neigh_agg_bwd.hip, as
include/pinsage_hip.h states them), their float64 closed forms with derived bounds, and the case table both test files share:
tests/test_agg_bwd_cases.py (CPU: the restatement against the closed forms and against torch autograd) and
tests/test_hip_agg_bwd.py (GPU: the kernels against the restatement, bit for bit).

Every fp32 product-and-add is oracle.pinsage_oracle._fmaf_vec (one rounding), every lane sum agg_cases.wave_sum; SEG is read
from the library (segment())."""
import functools

import numpy as np

from helpers import agg_cases as ac

U32 = 2.0 ** -24                            # unit roundoff of fp32
DW_ROWS = 128                               # target rows per partition of the dw2 sum (include/pinsage_hip.h)


def segment():
    """SEG = ps_gather_bwd_segment(): a compile-time constant of the library (no GPU needed to ask)"""
    from pinsage_hip import native
    return int(native.lib().ps_gather_bwd_segment())


def _f(a):
    return np.asarray(a, dtype=np.float32)


def _fma(a, b, c):
    from oracle.pinsage_oracle import _fmaf_vec
    a, b, c = np.broadcast_arrays(_f(a), _f(b), _f(c))
    return _fmaf_vec(a, b, c)


# ---- keep rules, slot lists ------------------------------------------------------------------------------------------------
def kept_pool(ids, nvalid, max_idx):
    """ps_importance_pool's keep rule: j < min(nvalid, T), 0 <= id <= max_idx"""
    ids = np.asarray(ids, dtype=np.int64)
    T = ids.shape[1]
    k = np.clip(np.asarray(nvalid, dtype=np.int64), 0, T)
    return (np.arange(T)[None, :] < k[:, None]) & (ids >= 0) & (ids <= max_idx)


def slot_lists_ref(ids, keep, n_rows):
    """(rptr int64[n_rows + 1], slots int32[nnz]): per feature row the kept slots s = i * T + j naming it, ascending"""
    ids = np.asarray(ids, dtype=np.int64)
    lists = [[] for _ in range(n_rows)]
    B, T = ids.shape
    for i in range(B):
        for j in range(T):
            if keep[i, j]:
                lists[ids[i, j]].append(i * T + j)
    rptr = np.zeros(n_rows + 1, dtype=np.int64)
    rptr[1:] = np.cumsum([len(l) for l in lists])
    slots = np.array([s for l in lists for s in l], dtype=np.int32)
    return rptr, slots


# ---- ps_pool_weights -------------------------------------------------------------------------------------------------------
def _tree(a):
    a = _f(a)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def pool_weights_exact(ids, counts, wts, nvalid, max_idx, renorm, lanes):
    """fp32 [B,T]: the weight ps_importance_pool applies to every slot.  w = fp32(fp64(count) / fp64(total)) with total the int32
    sum of counts[i, :k] (or the given weight), +0 where not kept; their sum: entry e sits in lane e % L (L = 16 for lanes == 16
    and T <= 64, else 64), a lane adds its entries in ascending order from +0, the L lanes are added by a balanced binary tree;
    with renorm and a positive sum every kept weight is divided by it (IEEE fp32)."""
    ids = np.asarray(ids)
    B, T = ids.shape
    L = 16 if lanes == 16 and T <= 64 else 64
    k = np.clip(np.asarray(nvalid, dtype=np.int64), 0, T)
    keep = kept_pool(ids, nvalid, max_idx)
    out = np.zeros((B, T), dtype=np.float32)
    for i in range(B):
        if wts is not None:
            w = _f(wts[i]).copy()
        else:
            tot = np.int32(np.asarray(counts[i, :k[i]], dtype=np.int64).sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                w = (np.asarray(counts[i], dtype=np.float64) / np.float64(tot)).astype(np.float32)
        w = np.where(keep[i], w, np.float32(0.0)).astype(np.float32)
        lane = np.zeros(L, dtype=np.float32)
        for e in range(T):
            lane[e % L] = lane[e % L] + w[e]
        wsum = _tree(lane)
        if renorm and wsum > 0:
            w = np.where(keep[i], w / wsum, np.float32(0.0)).astype(np.float32)
        out[i] = w
    return out


# ---- ps_gather_bwd / ps_attention_bwd_cols ---------------------------------------------------------------------------------
def _segmented(rptr, slots, n_rows, H, seg, term):
    """gx[r] = ((p_0 + p_1) + p_2) + ... over the SEG-slot segments of S(r), each p its own chain from +0 through term(acc, s)"""
    gx = np.zeros((n_rows, H), dtype=np.float32)
    for r in range(n_rows):
        lo, hi = int(rptr[r]), int(rptr[r + 1])
        total = None
        for p0 in range(lo, hi, seg):
            acc = np.zeros(H, dtype=np.float32)
            for s in slots[p0:min(p0 + seg, hi)]:
                acc = term(acc, int(s), r)
            total = acc if total is None else total + acc
        if total is not None:
            gx[r] = total
    return gx


def gather_bwd_exact(rptr, slots, n_rows, T, g, coef=None, arg=None, seg=None):
    """ps_gather_bwd: coef -> acc = fmaf(coef[s], g[s // T, c], acc); arg -> acc = acc + g[i, c] where arg[i, c] == j"""
    g = _f(g)
    seg = segment() if seg is None else seg
    assert (coef is None) != (arg is None)
    if coef is not None:
        cf = _f(coef).reshape(-1)
        return _segmented(rptr, slots, n_rows, g.shape[1], seg, lambda acc, s, r: _fma(cf[s], g[s // T], acc))
    arg = np.asarray(arg)
    return _segmented(rptr, slots, n_rows, g.shape[1], seg,
                      lambda acc, s, r: np.where(arg[s // T] == s % T, acc + g[s // T], acc).astype(np.float32))


def attention_bwd_cols_exact(rptr, slots, n_rows, T, ds, u, v, w2, seg=None):
    """ps_attention_bwd_cols: acc = fmaf(ds[s], (u[i, c] + v[r, c] > 0 ? w2[c] : 0), acc), the sum u + v rounded to fp32"""
    ds, u, v, w2 = _f(ds).reshape(-1), _f(u), _f(v), _f(w2)
    seg = segment() if seg is None else seg
    return _segmented(rptr, slots, n_rows, v.shape[1], seg,
                      lambda acc, s, r: _fma(ds[s], np.where(u[s // T] + v[r] > 0, w2, np.float32(0.0)), acc))


# ---- ps_gather_max_arg -----------------------------------------------------------------------------------------------------
def gather_max_arg_ref(x, ids, nvalid):
    """(out, arg): out = agg_cases.gather_max_ref; arg[i, c] = the lowest kept slot holding a NaN, else the lowest kept slot whose
    value equals the maximum, -1 for a row that keeps nothing"""
    x = _f(x)
    ids = np.asarray(ids)
    keep = ac.kept(ids, nvalid, x.shape[0])
    B, H = keep.shape[0], x.shape[1]
    out = np.zeros((B, H), dtype=np.float32)
    arg = np.full((B, H), -1, dtype=np.int32)
    for i in range(B):
        js = np.nonzero(keep[i])[0]
        if not js.size:
            continue
        rows = x[ids[i, js]]                                    # [k, H]
        nan = np.isnan(rows)
        with np.errstate(invalid="ignore"):
            mx = np.where(nan.any(axis=0), np.float32(np.nan), rows.max(axis=0))
        out[i] = mx
        hit = np.where(nan.any(axis=0)[None, :], nan, rows == mx[None, :])
        arg[i] = js[hit.argmax(axis=0)]
    return out, arg


# ---- ps_attention_bwd_rows -------------------------------------------------------------------------------------------------
def _lane_dot(a, b, vec):
    """[..., C] x [..., C] -> [...]: lane l chains part = fmaf(a[c], b[c], part) over its columns c = 64 vec k + vec l + e (sweep k,
    element e ascending) from +0, columns past C entering as 0 * 0; the 64 lanes are added by ps_wave_sum_f32's tree"""
    a, b = np.broadcast_arrays(_f(a), _f(b))
    C = a.shape[-1]
    chunk = 64 * vec
    sweeps = -(-C // chunk)

    def pad(t):
        out = np.zeros(t.shape[:-1] + (sweeps * chunk,), dtype=np.float32)
        out[..., :C] = t
        return out.reshape(t.shape[:-1] + (sweeps, 64, vec))
    ap, bp = pad(a), pad(b)
    part = np.zeros(a.shape[:-1] + (64,), dtype=np.float32)
    for k in range(sweeps):
        for e in range(vec):
            part = _fma(ap[..., k, :, e], bp[..., k, :, e], part)
    return ac.wave_sum(part)


def dw2_sum_exact(share):
    """[B, Hd] -> [Hd]: partitions of DW_ROWS consecutive rows, each acc = acc + share_i ascending from +0; then the partitions
    ascending from +0"""
    share = _f(share)
    B, Hd = share.shape
    total = np.zeros(Hd, dtype=np.float32)
    for r0 in range(0, B, DW_ROWS):
        acc = np.zeros(Hd, dtype=np.float32)
        for i in range(r0, min(r0 + DW_ROWS, B)):
            acc = acc + share[i]
        total = total + acc
    return total


def attention_bwd_rows_exact(x, u, v, w2, ids, nvalid, attn, g, vec):
    """(ds [B,T], du [B,Hd], dw2 [Hd], da [B,T]) of ps_attention_bwd_rows; vec: 4 when H % 4 == 0, Hd % 4 == 0 and the float
    operands are 16-byte aligned, else 1"""
    x, u, v, w2, attn, g = (_f(a) for a in (x, u, v, w2, attn, g))
    ids = np.asarray(ids)
    keep = ac.kept(ids, nvalid, v.shape[0])
    B, T = keep.shape
    Hd = v.shape[1]
    ds = np.zeros((B, T), dtype=np.float32)
    da = np.zeros((B, T), dtype=np.float32)
    du = np.zeros((B, Hd), dtype=np.float32)
    share = np.zeros((B, Hd), dtype=np.float32)
    zero = np.float32(0.0)
    for i in range(B):
        js = np.nonzero(keep[i])[0]
        if not js.size:
            continue
        da[i, js] = _lane_dot(g[i][None, :], x[ids[i, js]], vec)
        dot = np.zeros((), dtype=np.float32)
        for j in js:
            dot = _fma(attn[i, j], da[i, j], dot)
        ds[i, js] = attn[i, js] * (da[i, js] - dot)
        adu = np.zeros(Hd, dtype=np.float32)
        adw = np.zeros(Hd, dtype=np.float32)
        for j in js:
            h = u[i] + v[ids[i, j]]
            adu = _fma(ds[i, j], np.where(h > 0, w2, zero), adu)
            adw = _fma(ds[i, j], np.where(h < 0, zero, h), adw)
        du[i], share[i] = adu, adw
    return ds, du, dw2_sum_exact(share), da


# ---- float64 closed forms and bounds ---------------------------------------------------------------------------------------
def gather_bwd_64(ids, keep, n_rows, g, coef):
    """(gx, mag) in float64: gx[r] = sum over the kept slots naming r of coef[i, j] g[i]; mag the same sum of absolute values"""
    g, coef = np.asarray(g, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    gx = np.zeros((n_rows, g.shape[1]))
    mag = np.zeros_like(gx)
    for i, j in zip(*np.nonzero(keep)):
        gx[ids[i, j]] += coef[i, j] * g[i]
        mag[ids[i, j]] += np.abs(coef[i, j] * g[i])
    return gx, mag


def chain_bound(n_terms, mag):
    """a chain (or any tree) of n rounded additions of n products: (n + 2) u sum |terms|, the first-order bound of
    tests/helpers/gcn_cases.py (terms x unit roundoff x magnitude) with two spare roundings, plus the smallest subnormal"""
    return (np.asarray(n_terms, dtype=np.float64) + 2.0) * U32 * mag + 2.0 ** -149


def attention_grads_64(x, u, v, w2, ids, nvalid, g):
    """float64 gradients of out = sum_j softmax_j(w2 . relu(u_i + v_id)) x_id with respect to x, u, v, w2, from the formulas (not
    from autograd): dict(dx, du, dv, dw2, ds, attn, hmin) -- hmin = min |u + v| over kept slots and columns"""
    x, u, v, w2, g = (np.asarray(a, dtype=np.float64) for a in (x, u, v, w2, g))
    ids = np.asarray(ids)
    keep = ac.kept(ids, nvalid, v.shape[0])
    B, T = keep.shape
    attn = ac.attention_weights_ref(u, v, w2, ids, nvalid)
    dx, dv = np.zeros_like(x), np.zeros_like(v)
    du, dw2, ds = np.zeros_like(u), np.zeros_like(w2), np.zeros((B, T))
    hmin = np.inf
    for i in range(B):
        js = np.nonzero(keep[i])[0]
        if not js.size:
            continue
        nid = ids[i, js]
        da = x[nid] @ g[i]
        dsi = attn[i, js] * (da - attn[i, js] @ da)
        ds[i, js] = dsi
        h = u[i][None, :] + v[nid]
        hmin = min(hmin, np.abs(h).min())
        m = (h > 0) * w2[None, :]
        du[i] = dsi @ m
        dw2 += dsi @ np.maximum(h, 0.0)
        np.add.at(dv, nid, dsi[:, None] * m)
        np.add.at(dx, nid, attn[i, js][:, None] * g[i][None, :])
    return dict(dx=dx, du=du, dv=dv, dw2=dw2, ds=ds, attn=attn, hmin=hmin)


def attention_bounds(x, u, v, w2, ids, nvalid, attn32, g):
    """How far the exact-order fp32 results may lie from float64 formulas evaluated on the SAME fp32 attn (so the forward's
    error is not part of it).  With k_i kept slots, C columns, u = 2^-24:
      da   : C products through a lane chain and six tree levels: (C + 8) u sum_c |g x|                               =: e_da
      dot  : sum_j a_j (da_j + e_da_j), k fmaf: sum_j a_j e_da_j + (k + 2) u sum_j |a_j da_j|                            =: e_dot
      ds   : a (da - dot) with two roundings: a (e_da + e_dot) + 2 u a (|da| + |dot|)                                    =: e_ds
      du   : sum_j ds_j m_j: sum_j e_ds_j |w2| + (k + 2) u sum_j |ds_j| |w2|
      dw2  : sum_ij ds_ij relu(h), relu(h) itself rounded once: sum e_ds h+ + (k + DW_ROWS + P + 3) u sum |ds| h+
      dv_r : sum over S(r): sum e_ds |w2| + (n_r + nseg_r + 2) u sum |ds| |w2|
    Returns dict(ds, du, dv, dw2) of bounds and the float64 values dict(ds, du, dv, dw2) they are centred on."""
    x, u, v, w2, g, a = (np.asarray(t, dtype=np.float64) for t in (x, u, v, w2, g, attn32))
    ids = np.asarray(ids)
    keep = ac.kept(ids, nvalid, v.shape[0])
    B, T = keep.shape
    C = x.shape[1]
    seg = segment()
    val = dict(ds=np.zeros((B, T)), du=np.zeros_like(u), dv=np.zeros_like(v), dw2=np.zeros_like(w2))
    bnd = dict(ds=np.zeros((B, T)), du=np.zeros_like(u), dv=np.zeros_like(v), dw2=np.zeros_like(w2))
    dv_mag = np.zeros_like(v)
    dw_mag = np.zeros_like(w2)
    count = np.zeros(v.shape[0])
    P = -(-B // DW_ROWS)
    kmax = 0
    for i in range(B):
        js = np.nonzero(keep[i])[0]
        if not js.size:
            continue
        k = js.size
        kmax = max(kmax, k)
        nid = ids[i, js]
        da = x[nid] @ g[i]
        e_da = (C + 8) * U32 * (np.abs(x[nid]) @ np.abs(g[i]))
        dot = a[i, js] @ da
        e_dot = a[i, js] @ e_da + (k + 2) * U32 * (a[i, js] @ np.abs(da))
        dsi = a[i, js] * (da - dot)
        e_ds = a[i, js] * (e_da + e_dot) + 2 * U32 * a[i, js] * (np.abs(da) + abs(dot)) + 2.0 ** -149
        val["ds"][i, js], bnd["ds"][i, js] = dsi, e_ds
        h = u[i][None, :] + v[nid]
        m = (h > 0) * w2[None, :]
        hp = np.maximum(h, 0.0)
        val["du"][i] = dsi @ m
        bnd["du"][i] = e_ds @ np.abs(m) + (k + 2) * U32 * (np.abs(dsi) @ np.abs(m)) + 2.0 ** -149
        val["dw2"] += dsi @ hp
        bnd["dw2"] += e_ds @ hp
        dw_mag += np.abs(dsi) @ hp
        np.add.at(val["dv"], nid, dsi[:, None] * m)
        np.add.at(bnd["dv"], nid, e_ds[:, None] * np.abs(m))
        np.add.at(dv_mag, nid, np.abs(dsi)[:, None] * np.abs(m))
        np.add.at(count, nid, 1.0)
    bnd["dw2"] += (kmax + DW_ROWS + P + 3) * U32 * dw_mag + 2.0 ** -149
    bnd["dv"] += ((count + np.ceil(count / seg) + 2) * U32)[:, None] * dv_mag + 2.0 ** -149
    return bnd, val


# ---- the case table --------------------------------------------------------------------------------------------------------
# (B, N, H, T, offset, note): offset = the float operands start one float into their storage (agg_cases.OFFSET_CASE's plant)
CASES = (
    (50, 97, 33, 10, 0, "scalar sweep"),
    (50, 97, 64, 16, 0, "one 16-byte sweep, T = 16 edge"),
    (50, 97, 260, 17, 0, "second, partial 16-byte sweep; T = 17"),
    (50, 97, 64, 70, 0, "T > 64"),
    (1, 97, 64, 1, 0, "one row, one slot"),
    (50, 97, 64, 10, 1, "scalar sweep from alignment"),
    (50, 97, 33, 70, 0, "scalar sweep with T > 64"),
    (0, 97, 64, 10, 0, "empty batch"),
)
# The hub shape B = 2 SEG + 3, T = 2 has 4 SEG + 6 slots, fewer than the (SEG - 1) + SEG + (SEG + 1) + (2 SEG + 3) the four
# planted lengths need together (for any SEG > 3), so it comes as two batches: both give feature row 3 all 2 SEG + 3 slots of
# column 0; case(HUB_CASE) adds rows of SEG + 1 and SEG - 1 slots, case(HUB_CASE + 1) a row of exactly SEG.
HUB_CASE = len(CASES)
N_CASES = len(CASES) + 2


def _vec(H, offset):
    return 4 if H % 4 == 0 and not offset else 1


@functools.lru_cache(maxsize=None)
def case(ci):
    """Inputs of case ci (made once, shared, read-only).  x / v [N,H], u / g [B,H], w2 [H], counts / wts [B,T], ids / nvalid with
    planted rows (B = 50): feature rows 90 .. 94 are named by exactly 0, 1, 7, 8, 9 kept slots (nothing else names them);
    row 3 holds one id three times; row 5 holds -1, N and an id above max_idx below nvalid; nvalid of rows 7, 8, 9 is 0, T + 5
    and -3; feature rows 80 .. 83 are negative throughout and row 11 names only those (the maximum starts from -inf);
    feature rows 84 and 85 are equal (a max tie across distinct ids) and row 13 names 85 before 84.  max_idx = N - 3.
    The hub cases: feature rows 0, 2, 3 (first batch) and 1, 3 (second) are named by SEG - 1, SEG + 1, 2 SEG + 3 and SEG, 2 SEG + 3
    slots."""
    rs = np.random.RandomState(8800 + ci)
    if ci >= HUB_CASE:
        seg = segment()
        B, N, H, T, offset = 2 * seg + 3, 97, 64, 2, 0
    else:
        B, N, H, T, offset, _ = CASES[ci]
    x = rs.standard_normal((N, H)).astype(np.float32)
    v = rs.standard_normal((N, H)).astype(np.float32)
    u = rs.standard_normal((B, H)).astype(np.float32)
    g = rs.standard_normal((B, H)).astype(np.float32)
    w2 = (rs.uniform(-1.0, 1.0, H) / np.sqrt(H)).astype(np.float32)
    counts = rs.randint(1, 30, size=(B, T)).astype(np.int32)
    wts = (rs.random_sample((B, T)) + 0.05).astype(np.float32)
    x[80:84] = -np.abs(x[80:84]) - np.float32(0.5)
    x[85] = x[84]
    if ci >= HUB_CASE:
        # column 0 of every row names feature row 3; column 1 shares out its 2 SEG + 3 slots
        ids = np.full((B, T), -1, dtype=np.int32)
        nvalid = np.full(B, T, dtype=np.int32)
        ids[:, 0] = 3
        if ci == HUB_CASE:
            ids[:seg + 1, 1] = 2
            ids[seg + 1:2 * seg, 1] = 0
        else:
            ids[2:seg + 2, 1] = 1
            ids[seg + 2:, 1] = rs.randint(4, 80, size=B - seg - 2)
    else:
        ids = rs.randint(0, 80, size=(B, T)).astype(np.int32)
        nvalid = rs.randint(1, T + 1, size=B).astype(np.int32)
        if B == 50:
            nvalid[20:] = T
            # planted destination rows 90..94 with 0, 1, 7, 8, 9 slots (column 0 of rows 20..44)
            plant = [91] * 1 + [92] * 7 + [93] * 8 + [94] * 9
            ids[20:20 + len(plant), 0] = plant
            if T >= 3:
                ids[3, :3] = 17
                nvalid[3] = T
                ids[5, :3] = [-1, N, N - 2]
                nvalid[5] = T
            else:
                ids[5, 0] = -1
            nvalid[7], nvalid[8], nvalid[9] = 0, T + 5, -3
            ids[11] = 80 + (np.arange(T) % 4)
            nvalid[11] = T
            ids[13, 0] = 85
            if T >= 2:
                ids[13, 1] = 84
            nvalid[13] = min(T, 2)
    out = dict(B=B, N=N, H=H, T=T, offset=offset, vec=_vec(H, offset), x=x, v=v, u=u, g=g, w2=w2, counts=counts, wts=wts,
               ids=ids, nvalid=nvalid, max_idx=N - 3)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
