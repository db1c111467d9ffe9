"""The case table of the attention / max-pool aggregator tests and a float64 restatement of what the reference's two
`forward`s compute (model/aggregators.py:113-160, 182-211), one python loop per output row, written from their description:

  attention   for a row with neighbours n_1..n_k: s_j = W2 relu(W1 cat(self_i, x[n_j]) + b1) + b2, a = softmax(s) over the
              row's neighbours, out_i = sum_j a_j x[n_j]; zeros for a row without neighbours
  max-pool    out_i = max_j relu(W x[n_j] + b), per column; zeros for a row without neighbours

and of the two C entry points over padded (ids, nvalid) with their keep rule (include/pinsage_hip.h).  numpy only: shared by
tests/test_agg_cases.py (CPU) and tests/test_hip_aggregators.py (GPU).

GATE_CASES, further down, are the rows that reach the launcher gates of csrc/neigh_agg.hip which CASES leaves out (agg_facts /
plants restate the launcher for that proof, never for an expected value), with attention_scores_exact -- the kernel's fp32
score of every kept slot, bit for bit -- and attention_bound, the derived distance of its softmax from the fp64 softmax of those
scores: tests/test_hip_agg_matrix.py."""
import functools

import numpy as np

RTOL, ATOL = 1e-5, 2e-6                     # tests/test_hip_model.py's embedding tolerance

# (B, N, C, T, note)
CASES = (
    (1, 1, 1, 1, "single neighbour"),
    (5, 7, 3, 1, ""),
    (6, 12, 8, 5, "the G4 shape"),
    (33, 50, 10, 7, "scalar path"),
    (64, 400, 256, 50, "one full sweep"),
    (17, 90, 260, 64, "sweep tail, T = 64 edge"),
    (9, 80, 64, 70, "T > 64"),
    (40, 64, 512, 16, "two sweeps"),
    (20000, 300, 8, 2, "the grid-stride loop runs more than once"),
    (16, 40, 8, 4, "x, u, v at a one-float storage offset: contiguous, not 16-byte aligned"),
    (7, 30, 6, 70, "scalar path with T > 64 (beyond the issue's table)"),
)
OFFSET_CASE = 9                             # its float operands are placed one float into their storage
SCALED_CASE = 4                             # the variant with the last attention layer x 8 runs on this case


def out_channels(ci):
    """MaxPoolingAggregator(C, out) of case ci: a multiple of four (16 B sweeps) on the even cases, not on most odd ones"""
    C = CASES[ci][2]
    return C if ci % 2 == 0 else C // 2 + 1


@functools.lru_cache(maxsize=None)
def case(ci):
    """Inputs of case ci (made once, shared, read-only):
      x [N,C], self_x [B,C]          N(0,1) features / target rows
      u [B,C], v [N,C], w2 [C]       operands of the raw attention entry point (w2 within the default nn.Linear bound 1/sqrt(C))
      nvalid [B]                     1, 0, T, random, ... by row
      ids [B,T]                      legal ids, -1 beyond nvalid (what the modules' padding makes); duplicates within a row
      raw_ids [B,T]                  for the raw entry points: junk beyond nvalid, and (all cases but the first) some slots below
                                     nvalid set to -1, N and 2^31 - 1; every eighth row loses all of its slots that way
      neighbors                      the python list-of-lists view of (ids, nvalid)"""
    B, N, C, T, _ = CASES[ci]
    rs = np.random.RandomState(4100 + ci)
    x = rs.standard_normal((N, C)).astype(np.float32)
    self_x = rs.standard_normal((B, C)).astype(np.float32)
    u = rs.standard_normal((B, C)).astype(np.float32)
    v = rs.standard_normal((N, C)).astype(np.float32)
    w2 = (rs.uniform(-1.0, 1.0, C) / np.sqrt(C)).astype(np.float32)
    nvalid = np.empty(B, dtype=np.int32)
    nvalid[0::4] = 1
    nvalid[1::4] = 0
    nvalid[2::4] = T
    nvalid[3::4] = rs.randint(0, T + 1, size=len(nvalid[3::4]))
    ids = rs.randint(0, N, size=(B, T)).astype(np.int32)
    if T >= 3:                                                                         # a duplicate in every row of three or more
        ids[:, 2] = np.where(nvalid >= 3, ids[:, 0], ids[:, 2])
    elif T == 2:                                                                       # T = 2: in every eighth row (elsewhere the
        ids[2::8, 1] = ids[2::8, 0]                                                    # two neighbours differ, so the weights matter)
    slot = np.arange(T)[None, :]
    inrow = slot < nvalid[:, None]
    raw = ids.copy()
    junk = np.array([-1, N, 2 ** 31 - 1, 0, N - 1, -(2 ** 31)], dtype=np.int64)
    raw[~inrow] = junk[rs.randint(0, len(junk), size=int((~inrow).sum()))].astype(np.int32)
    if ci != 0:
        bad = np.array([-1, N, 2 ** 31 - 1], dtype=np.int64).astype(np.int32)
        for i in range(B):
            k = int(nvalid[i])
            if i % 8 == 6:
                raw[i, :k] = bad[np.arange(k) % 3]                                         # a row with slots that keeps nothing
            elif k >= 2 and i % 3 == 0:
                raw[i, i % k] = bad[(i // 3) % 3]
    ids[~inrow] = -1
    neighbors = [[int(t) for t in ids[i, :nvalid[i]]] for i in range(B)]
    out = dict(B=B, N=N, C=C, T=T, x=x, self_x=self_x, u=u, v=v, w2=w2, nvalid=nvalid, ids=ids, raw_ids=raw, neighbors=neighbors)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def kept(ids, nvalid, N):
    """bool[B,T]: slot j of row i is kept iff j < min(nvalid[i], T) and 0 <= ids[i,j] < N"""
    ids = np.asarray(ids, dtype=np.int64)
    T = ids.shape[1]
    k = np.clip(np.asarray(nvalid, dtype=np.int64), 0, T)
    return (np.arange(T)[None, :] < k[:, None]) & (ids >= 0) & (ids < N)


def _softmax64(s):
    e = np.exp(s - s.max())
    return e / e.sum()


def attention_weights_ref(u, v, w2, ids, nvalid):
    """ps_attention_weights in float64: attn[B,T], zeros where a slot is not kept"""
    u, v, w2 = (np.asarray(a, dtype=np.float64) for a in (u, v, w2))
    keep = kept(ids, nvalid, v.shape[0])
    attn = np.zeros(keep.shape, dtype=np.float64)
    for i in range(keep.shape[0]):
        js = np.nonzero(keep[i])[0]
        if js.size:
            s = np.maximum(u[i][None, :] + v[np.asarray(ids[i])[js]], 0.0) @ w2
            attn[i, js] = _softmax64(s)
    return attn


def gather_max_ref(x, ids, nvalid):
    """ps_gather_max in x's own dtype (a maximum has no rounding): NaN propagates, zeros for a row that keeps nothing"""
    x = np.asarray(x)
    keep = kept(ids, nvalid, x.shape[0])
    out = np.zeros((keep.shape[0], x.shape[1]), dtype=x.dtype)
    for i in range(keep.shape[0]):
        js = np.nonzero(keep[i])[0]
        if js.size:
            out[i] = x[np.asarray(ids[i])[js]].max(axis=0)
    return out


def attention_forward_ref(features, neighbors, W1, b1, W2, b2, self_features=None):
    """AttentionAggregator.forward in float64"""
    f, W1, b1, W2, b2 = (np.asarray(a, dtype=np.float64) for a in (features, W1, b1, W2, b2))
    sf = f if self_features is None else np.asarray(self_features, dtype=np.float64)
    out = np.zeros((len(neighbors), f.shape[1]), dtype=np.float64)
    for i, nb in enumerate(neighbors):
        if len(nb) == 0:
            continue
        nf = f[np.asarray(nb, dtype=np.int64)]
        cat = np.concatenate([np.broadcast_to(sf[i], nf.shape), nf], axis=1)
        s = (np.maximum(cat @ W1.T + b1, 0.0) @ W2.T + b2)[:, 0]
        out[i] = (nf * _softmax64(s)[:, None]).sum(axis=0)
    return out


def maxpool_forward_ref(features, neighbors, W, b):
    """MaxPoolingAggregator.forward in float64"""
    f, W, b = (np.asarray(a, dtype=np.float64) for a in (features, W, b))
    out = np.zeros((len(neighbors), W.shape[0]), dtype=np.float64)
    for i, nb in enumerate(neighbors):
        if len(nb):
            out[i] = np.maximum(f[np.asarray(nb, dtype=np.int64)] @ W.T + b, 0.0).max(axis=0)
    return out


def modules(ci, scaled=False):
    """(AttentionAggregator(C), MaxPoolingAggregator(C, out_channels(ci))) of case ci on the CPU, in eval mode, with torch's
    default nn.Linear initialisation seeded per case; scaled: the last attention layer x 8"""
    import torch
    from model import aggregators as A
    C = CASES[ci][2]
    torch.manual_seed(7700 + ci)
    at, mp = A.AttentionAggregator(C), A.MaxPoolingAggregator(C, out_channels(ci))
    if scaled:
        with torch.no_grad():
            at.attention[2].weight.mul_(8.0)
            at.attention[2].bias.mul_(8.0)
    return at.eval(), mp.eval()


def at_ref(at, features, neighbors, self_features=None):
    p = {k: t.detach().cpu().numpy() for k, t in at.state_dict().items()}
    return attention_forward_ref(features, neighbors, p["attention.0.weight"], p["attention.0.bias"], p["attention.2.weight"],
                                 p["attention.2.bias"], self_features)


def mp_ref(mp, features, neighbors):
    p = {k: t.detach().cpu().numpy() for k, t in mp.state_dict().items()}
    return maxpool_forward_ref(features, neighbors, p["mlp.0.weight"], p["mlp.0.bias"])


# ---- the launcher gates CASES does not reach -----------------------------------------------------------------------------------
# (B, N, C, T, offset, gate): offset = the float operands start one float past a 16-byte boundary
GATE_CASES = (
    (9, 40, 65, 3, 0, "scalar path, second sweep of one column"),
    (9, 40, 130, 5, 0, "scalar path, three sweeps"),
    (6, 40, 256, 4, 1, "scalar path from alignment, four sweeps"),
    (5, 90, 8, 65, 0, "one slot in a second slot block"),
    (5, 200, 8, 130, 0, "three slot blocks, vector path"),
    (5, 200, 6, 130, 0, "three slot blocks, scalar path"),
)
PLANTED = ("over", "huge", "twin", "neg", "negmin", "late", "one")      # the planted rows, the last seven of every gate case
UNROLL = 8                                  # csrc/neigh_agg.hip
ROW_GRID_CAP = 256 * 16                     # ps_row_grid() (csrc/ps_common.h): workgroups of four waves


def _cdiv(a, b):
    return -(-a // b)


def agg_facts(B, N, C, T, offset=0):
    """ps_attention_weights' launcher and loop bounds restated (coverage proofs and messages only)"""
    vec = 4 if C % 4 == 0 and not offset else 1
    grid = min(_cdiv(B, 4), ROW_GRID_CAP)
    return dict(vec=vec, sweeps=_cdiv(C, 64 * vec), slot_blocks=_cdiv(T, 64), small=T <= 64, grid=grid, passes=_cdiv(B, 4 * grid))


def plants(ids, nvalid, N):
    """what the rows of (ids, nvalid) plant: nvalid beyond T, negative nvalid, and -- T > 64 -- a row whose first 64 slots are all
    dropped and which keeps a later one"""
    ids, nvalid = np.asarray(ids), np.asarray(nvalid, dtype=np.int64)
    T = ids.shape[1]
    keep = kept(ids, nvalid, N)
    late = T > 64 and bool((~keep[:, :64].any(axis=1) & keep[:, 64:].any(axis=1)).any())
    return dict(over=bool((nvalid > T).any()), negative=bool((nvalid < 0).any()), late=late)


# name -> predicate over (agg_facts, plants): the gates tests/test_agg_cases.py shows CASES not to reach and GATE_CASES to reach
AGG_GATES = {
    "attention_weights_kernel<1>: c0 != 0 reloads u and w2": lambda f, p: f["vec"] == 1 and f["sweeps"] >= 2,
    "three or more 64-slot blocks": lambda f, p: f["slot_blocks"] >= 3,
    "nvalid > T": lambda f, p: p["over"],
    "nvalid < 0": lambda f, p: p["negative"],
    "T > 64: the first slot block keeps nothing, a later one does": lambda f, p: p["late"],
}


@functools.lru_cache(maxsize=None)
def gate_case(gi):
    """Inputs of GATE_CASES[gi], as case(): x, self-free operands u, v, w2, raw ids / nvalid for the two raw entry points.  The
    rows are max(B - 7, 2) ordinary ones (row 0 keeps all T slots, the others a random count with one slot dropped) and seven
    planted ones, `rows[name]` (rows are added where B is too small for them):
      over, huge, twin   the same ids (one slot dropped for T >= 3) under nvalid = T + 5, 2^31 - 1 and T: equal results
      neg, negmin        nvalid = -1 and -2^31 over legal ids: nothing is kept
      late               T > 64: slots 0..63 hold -1, N, 2^31 - 1 and the kept slots come after them (T <= 64: one neighbour)
      one                every kept slot names the same neighbour (one slot dropped for T >= 3): weights of exactly 1 / n"""
    B, N, C, T, offset, _ = GATE_CASES[gi]
    rs = np.random.RandomState(5200 + gi)
    plain = max(B - len(PLANTED), 2)
    Bt = plain + len(PLANTED)
    x = rs.standard_normal((N, C)).astype(np.float32)
    u = rs.standard_normal((Bt, C)).astype(np.float32)
    v = rs.standard_normal((N, C)).astype(np.float32)
    w2 = (rs.uniform(-1.0, 1.0, C) / np.sqrt(C)).astype(np.float32)
    bad = np.array([-1, N, 2 ** 31 - 1], dtype=np.int64).astype(np.int32)
    ids = rs.randint(0, N, size=(Bt, T)).astype(np.int32)
    nvalid = np.full(Bt, T, dtype=np.int32)
    for i in range(1, plain):
        nvalid[i] = rs.randint(1, T + 1)
        ids[i, nvalid[i]:] = bad[np.arange(T - nvalid[i]) % 3]
        if nvalid[i] >= 2:
            ids[i, i % nvalid[i]] = bad[i % 3]
    rows = {name: plain + k for k, name in enumerate(PLANTED)}
    if T >= 3:
        ids[rows["over"], T // 2] = bad[2]
    ids[rows["huge"]] = ids[rows["twin"]] = ids[rows["over"]]
    u[rows["huge"]] = u[rows["twin"]] = u[rows["over"]]
    nvalid[rows["over"]], nvalid[rows["huge"]] = T + 5, 2 ** 31 - 1
    nvalid[rows["neg"]], nvalid[rows["negmin"]] = -1, -(2 ** 31)
    if T > 64:
        ids[rows["late"], :64] = bad[np.arange(64) % 3]
    else:
        nvalid[rows["late"]] = 1
    ids[rows["one"]] = rs.randint(0, N)
    if T >= 3:
        ids[rows["one"], 1] = -1
    out = dict(B=Bt, N=N, C=C, T=T, offset=offset, x=x, u=u, v=v, w2=w2, nvalid=nvalid, raw_ids=ids, rows=rows,
               vec=agg_facts(Bt, N, C, T, offset)["vec"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def wave_sum(lanes):
    """ps_wave_sum_f32 of fp32 [..., 64]: a balanced binary tree over the lanes in their order (tests/helpers/bn_cases.py)"""
    a = np.asarray(lanes, dtype=np.float32)
    assert a.shape[-1] == 64
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def attention_scores_exact(u, v, w2, ids, nvalid, vec, sequential=False):
    """fp32 [B, T]: ps_attention_weights' score of every kept slot, -inf elsewhere, in the kernel's order: lane l chains
    part = fmaf(w2[c], relu(u[c] + v[c]), part) over its columns k * 64 * vec + l * vec + e (sweep k, element e, ascending) from
    +0.0, the sum u + v rounded and relu as h < 0 -> +0.0; the 64 lanes are then added by ps_wave_sum_f32's balanced tree.  vec:
    4 when C % 4 == 0 and u, v, w2 are 16-byte aligned, else 1.  sequential: the near miss that adds the lanes one after the
    other."""
    from oracle.pinsage_oracle import _fmaf_vec
    u, v, w2 = (np.asarray(a, dtype=np.float32) for a in (u, v, w2))
    ids = np.asarray(ids)
    C = v.shape[1]
    chunk = 64 * vec
    sweeps = _cdiv(C, chunk)

    def pad(a):                                           # a column past C: fmaf(0, relu(0 + 0), part) = part (part is never -0.0)
        out = np.zeros(a.shape[:-1] + (sweeps * chunk,), dtype=np.float32)
        out[..., :C] = a
        return out.reshape(a.shape[:-1] + (sweeps, 64, vec))
    keep = kept(ids, nvalid, v.shape[0])
    scores = np.full(keep.shape, -np.inf, dtype=np.float32)
    wp = pad(w2)
    for i in range(keep.shape[0]):
        js = np.nonzero(keep[i])[0]
        if not js.size:
            continue
        h = pad(u[i])[None] + pad(v[ids[i, js]])          # fp32, rounded
        h = np.where(h < 0, np.float32(0.0), h)
        part = np.zeros((js.size, 64), dtype=np.float32)
        for k in range(sweeps):
            for e in range(vec):
                part = _fmaf_vec(np.broadcast_to(wp[k, :, e], part.shape), h[:, k, :, e], part)
        if sequential:
            s = part[:, 0]
            for lane in range(1, 64):
                s = s + part[:, lane]
            scores[i, js] = s
        else:
            scores[i, js] = wave_sum(part)
    return scores


def softmax_of_scores(scores):
    """fp64 [B, T]: the softmax of fp32 scores over the slots that are not -inf, every operation in fp64; zeros elsewhere"""
    s = np.asarray(scores, dtype=np.float64)
    out = np.zeros(s.shape, dtype=np.float64)
    for i in range(s.shape[0]):
        js = np.nonzero(np.isfinite(s[i]))[0]
        if js.size:
            out[i, js] = _softmax64(s[i, js])
    return out


# expf's error bound E in ulp: the measured maximum, 0.8164 ulp over the 18 043 arguments of GATE_CASES and CASES (in [-17.48, 0];
# profiles/expf_ulp_attention.txt, tools/expf_ulp.py on an MI355X with the library's compiler flags), rounded up, plus one ulp
EXPF_ULP = 0.82 + 1.0


def expf_arguments(scores):
    """fp32: the arguments s - max (rounded once, as the kernel subtracts) of the kept slots of a score table"""
    s = np.asarray(scores, dtype=np.float32)
    rows = np.isfinite(s).any(axis=1)
    with np.errstate(invalid="ignore"):
        d = s[rows] - s[rows].max(axis=1, keepdims=True)
    return d[np.isfinite(d)].astype(np.float32)


def attention_bound(scores, T):
    """fp64 [B, T]: how far ps_attention_weights' fp32 weight of a kept slot may lie from softmax_of_scores(scores), the fp64
    softmax of the kernel's own fp32 scores (attention_scores_exact).  With u = 2^-24 and a_j the reference weight of slot j:

      the maximum m is exact; d_j = fl(s_j - m) is rounded once, |d_j - (s_j - m)| <= |s_j - m| u, which multiplies the
      exponential by at most exp(|s_j - m| u) = 1 + |s_j - m| u to first order;
      expf returns its value within E ulp, a relative error of at most E 2^-23 = 2 E u (an ulp is at most 2^-23 of the value);
      so e_j carries delta_j = (|s_j - m| + 2 E) u;
      the sum of the e_j goes through at most D = ceil(T / 64) - 1 + 6 additions of non-negative terms (a lane's own slots one
      after the other, then the six steps of the wave sum), each with relative error u and none amplified -- all terms have one
      sign --, so the sum carries sum_k a_k delta_k + D u;
      the division is rounded once: u.

      |attn_j - a_j| <= a_j (delta_j + sum_k a_k delta_k + (D + 2) u) + 2^-149

    one u of the (D + 2) for the second-order terms -- the whole factor stays below 2^-12 here, its square below u / 2 -- and
    2^-149 for a quotient in the subnormal range.  The derivation needs exp(d_j) to be a normal number: scores more than 80
    apart within a row are refused.
    E = EXPF_ULP cannot be derived here, and no copy of HIP's math-accuracy table ships with the toolchain: it is measured by
    tools/expf_ulp.py, which runs one kernel that evaluates expf on exactly the arguments d_j of GATE_CASES and CASES and
    compares with fp64 exp of the same fp32 arguments on the host (the library function against the reference, not the kernel
    under test).  Measured maximum 0.8164 ulp (profiles/expf_ulp_attention.txt); E = that, rounded up, plus one ulp = 1.82."""
    s = np.asarray(scores, dtype=np.float64)
    u = 2.0 ** -24
    D = _cdiv(T, 64) - 1 + 6
    a = softmax_of_scores(scores)
    fin = np.isfinite(s)
    with np.errstate(invalid="ignore"):
        gap = np.where(fin, np.where(fin, s, -np.inf).max(axis=1, keepdims=True) - np.where(fin, s, 0.0), 0.0)
    assert (gap <= 80.0).all()
    delta = np.where(fin, (gap + 2.0 * EXPF_ULP) * u, 0.0)
    factor = delta + (a * delta).sum(axis=1, keepdims=True) + (D + 2) * u
    assert (factor < 2.0 ** -12).all()
    return np.where(fin, a * factor + 2.0 ** -149, 0.0)
