"""The case table of the attention / max-pool aggregator tests and a float64 restatement of what the reference's two
`forward`s compute (model/aggregators.py:113-160, 182-211), one python loop per output row, written from their description:

  attention   for a row with neighbours n_1..n_k: s_j = W2 relu(W1 cat(self_i, x[n_j]) + b1) + b2, a = softmax(s) over the
              row's neighbours, out_i = sum_j a_j x[n_j]; zeros for a row without neighbours
  max-pool    out_i = max_j relu(W x[n_j] + b), per column; zeros for a row without neighbours

and of the two C entry points over padded (ids, nvalid) with their keep rule (include/pinsage_hip.h).  numpy only: shared by
tests/test_agg_cases.py (CPU) and tests/test_hip_aggregators.py (GPU)."""
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
