"""What the model.layers tests share: the recorded reference outputs (tests/golden/reference_golden_layers.npz), a float64 numpy
restatement of the reference's four `forward`s (model/layers.py:44-77, 87-133, 143-195, 205-237) written from their description,
a float64 restatement of the two batch-norm entry points (include/pinsage_hip.h) and the inputs of their shape table.  numpy
only: shared by tests/test_layers_cases.py (CPU) and tests/test_hip_layers.py (GPU).

  GraphConvLayer   t = linear_out(cat[linear_self(x), linear_neigh(n)]); for more than one row t = bn(t) -- training: batch mean
                   and biased batch variance, running statistics moved by `momentum` towards the mean and the UNBIASED variance,
                   num_batches_tracked + 1; eval: the running statistics --; out = relu(t) / max(||relu(t)||_2, 1e-12) per row
  pooling layers   per list: ids >= N dropped, negative ids from the end; weights = the first len(kept) of the row's weights,
                   divided by their left-to-right sum (uniform / mean when that is 0); zeros for a row that keeps nothing"""
import functools
import os

import numpy as np

RTOL, ATOL = 1e-5, 2e-6                     # tests/test_hip_model.py's embedding tolerance
S = 128                                     # rows per partition of ps_bn_batch_stats (dense.BN_STATS_ROWS)
EPS, MOMENTUM = 1e-5, 0.1                   # nn.BatchNorm1d's defaults
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "reference_golden_layers.npz")

STATS_M = (2, 3, S - 1, S, S + 1, 70 * S + 3)
STATS_N = (1, 21, 64, 256, 260)
OFFSET_SHAPE = (S + 1, 260)                 # run a second time with z one float past a 16-byte boundary


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def state_dict(prefix, dtype=None):
    """the recorded state_dict `prefix` (init_, p_, r_) as numpy arrays; dtype: cast the float entries"""
    sd = {k[len(prefix):]: v for k, v in golden().items() if k.startswith(prefix) and "." in k}
    assert len(sd) == 11, sorted(sd)
    return {k: (v.astype(dtype) if dtype is not None and v.dtype.kind == "f" else v) for k, v in sd.items()}


def golden_lists():
    """(neighbors, weights) of the pooling cases as python lists of ints / floats"""
    g = golden()
    nb = [[int(t) for t in g["pool_ids"][i, :g["pool_len"][i]]] for i in range(g["pool_ids"].shape[0])]
    w = [[float(t) for t in g["pool_w"][i, :g["pool_wlen"][i]]] for i in range(g["pool_w"].shape[0])]
    return nb, w


# ---- float64 restatements ------------------------------------------------------------------------------------------------------
def graph_conv_ref(sd, x, nx, training):
    """GraphConvLayer.forward in float64 over a state_dict of numpy arrays.  Returns (out, sd') where sd' holds the bn buffers
    after the call (sd itself is not changed)."""
    p = {k: np.asarray(v, dtype=np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v) for k, v in sd.items()}
    x, nx = np.asarray(x, dtype=np.float64), np.asarray(nx, dtype=np.float64)
    a = x @ p["linear_self.weight"].T + p["linear_self.bias"]
    b = nx @ p["linear_neigh.weight"].T + p["linear_neigh.bias"]
    t = np.concatenate([a, b], axis=1) @ p["linear_out.weight"].T + p["linear_out.bias"]
    M = t.shape[0]
    if M > 1:
        if training:
            mean, var = t.mean(axis=0), t.var(axis=0)
            p["bn.running_mean"] = (1 - MOMENTUM) * p["bn.running_mean"] + MOMENTUM * mean
            p["bn.running_var"] = (1 - MOMENTUM) * p["bn.running_var"] + MOMENTUM * var * M / (M - 1)
            p["bn.num_batches_tracked"] = p["bn.num_batches_tracked"] + 1
        else:
            mean, var = p["bn.running_mean"], p["bn.running_var"]
        t = (t - mean) / np.sqrt(var + EPS) * p["bn.weight"] + p["bn.bias"]
    t = np.maximum(t, 0.0)
    out = t / np.maximum(np.sqrt((t * t).sum(axis=1, keepdims=True)), 1e-12)
    return out, p


def _kept(nb, N):
    kept = [n for n in nb if n < N]
    for n in kept:
        if n < -N:
            raise IndexError(n)
    return [n + N if n < 0 else n for n in kept]


def _row_weights(w_row, k):
    """float32 weights of a row with k kept ids as float64 values; None: the plain mean"""
    nw = list(w_row[:k])
    s = sum(nw)
    if s == 0:
        return None
    return np.asarray([v / s for v in nw], dtype=np.float64).astype(np.float32).astype(np.float64)


def importance_pool_ref(x, neighbors, weights):
    x = np.asarray(x, dtype=np.float64)
    rows = []
    for nb, wr in zip(neighbors, weights):
        kept = _kept(nb, x.shape[0])
        if not kept:
            rows.append(np.zeros(x.shape[1]))
            continue
        w = _row_weights(wr, len(kept))
        if w is None:
            w = np.full(len(kept), np.float64(np.float32(1.0 / len(kept))))
        rows.append((x[kept] * w[:, None]).sum(axis=0))
    return np.stack(rows)


def weighted_mean_pool_ref(x, neighbors, weights=None):
    x = np.asarray(x, dtype=np.float64)
    rows = []
    for i, nb in enumerate(neighbors):
        kept = _kept(nb, x.shape[0])
        if not kept:
            rows.append(np.zeros(x.shape[1]))
            continue
        w = _row_weights(weights[i], len(kept)) if weights is not None and len(weights) > i else None
        rows.append(x[kept].mean(axis=0) if w is None else (x[kept] * w[:, None]).sum(axis=0))
    return np.stack(rows)


def max_pool_ref(x, neighbors):
    """in x's own dtype: a maximum has no rounding"""
    x = np.asarray(x)
    rows = []
    for nb in neighbors:
        kept = _kept(nb, x.shape[0])
        rows.append(x[kept].max(axis=0) if kept else np.zeros(x.shape[1], dtype=x.dtype))
    return np.stack(rows)


def bn_stats_ref(z, gamma, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM):
    """ps_bn_batch_stats in float64 on the fp32 z: dict of mean, var, scale, ez2 = E[z^2] (for the error bounds) and, when the
    running statistics are given, their new values rm / rv"""
    z = np.asarray(z, dtype=np.float64)
    M = z.shape[0]
    mean, ez2 = z.mean(axis=0), (z * z).mean(axis=0)
    var = ((z - mean) ** 2).mean(axis=0)                              # the two-pass formula: no cancellation
    out = {"mean": mean, "var": var, "ez2": ez2, "scale": np.asarray(gamma, dtype=np.float64) / np.sqrt(var + eps)}
    if running_mean is not None:
        out["rm"] = (1 - momentum) * np.asarray(running_mean, dtype=np.float64) + momentum * mean
        out["rv"] = (1 - momentum) * np.asarray(running_var, dtype=np.float64) + momentum * var * M / (M - 1)
    return out


def bn_apply_ref(z, mean, scale, beta, relu, l2norm):
    """ps_bn_apply in float64"""
    z, mean, scale, beta = (np.asarray(a, dtype=np.float64) for a in (z, mean, scale, beta))
    t = (z - mean) * scale + beta
    if relu:
        t = np.maximum(t, 0.0)
    if l2norm:
        t = t / np.maximum(np.sqrt((t * t).sum(axis=1, keepdims=True)), 1e-12)
    return t


# ---- inputs of the batch-norm shape table ----------------------------------------------------------------------------------------
CONST = np.float32(3.7)


@functools.lru_cache(maxsize=None)
def stats_case(M, N):
    """Inputs of shape (M, N), made once, shared, read-only:
      z [M,N]        N(0.3, 1.5) columns; column 0 has mean 100 and standard deviation 0.05 (E[z^2] / var = 4e6: a single-pass
                     fp32 E[z^2] - mean^2 has no correct digit there); for N >= 2 the last column is the constant CONST
      gamma, beta    bn.weight-like in (0.5, 1.5) / N(0, 0.5)
      rm0, rv0       running statistics before the call
      ap_mean, ap_scale   a mean / positive scale for the apply tests
      neg [N], neg_row    a row so far below ap_mean that (neg - ap_mean) * ap_scale + beta < 0 in every column, and where the
                     apply tests put it (the statistics tests take z as it is)"""
    rs = np.random.RandomState(1000 * N + M % 997)
    z = (0.3 + 1.5 * rs.standard_normal((M, N))).astype(np.float32)
    z[:, 0] = (100.0 + 0.05 * rs.standard_normal(M)).astype(np.float32)
    if N >= 2:
        z[:, N - 1] = CONST
    gamma = rs.uniform(0.5, 1.5, N).astype(np.float32)
    beta = (0.5 * rs.standard_normal(N)).astype(np.float32)
    rm0 = rs.standard_normal(N).astype(np.float32)
    rv0 = rs.uniform(0.5, 2.0, N).astype(np.float32)
    ap_mean = z.astype(np.float64).mean(axis=0).astype(np.float32)
    ap_scale = rs.uniform(0.5, 2.0, N).astype(np.float32)
    neg = ap_mean - (np.abs(beta) / ap_scale + 1.0 + np.abs(rs.standard_normal(N))).astype(np.float32)
    out = dict(M=M, N=N, z=z, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, ap_mean=ap_mean, ap_scale=ap_scale, neg_row=M // 2, neg=neg)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
