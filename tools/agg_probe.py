#!/usr/bin/env python3
"""Attention / max-pool aggregators: the HIP path (ps_linear + ps_attention_weights + ps_importance_pool; ps_linear +
ps_gather_max) against the batched torch code of the same commit (`_torch_padded`: what `_forward_torch` runs after padding), in
ONE process on one GPU, alternating.  Both take the same padded device tensors (ids int32 [B,T], nvalid int32 [B]); the python
padding of the list-of-lists API is common to both paths and is reported once per shape (`pad_ms`, host clock); the whole module
calls from python lists, `forward` against `_forward_torch`, are timed too (median of 3, host clock around a synchronise).  Per shape and
path: the median and minimum of `--reps` calls timed with HIP events after `--warmup` calls, and the rise of torch's peak
allocation over one call.  The two gather kernels are also timed alone; their rate is over the algorithmic bytes -- 4 C per kept
(row, slot), counted once per kernel.  Prints one JSON line (and writes it to --json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommendation-engine_amd"))
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from model import aggregators as A                             # noqa: E402
from pinsage_hip import dense, sampling                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rows", type=int, default=59047, help="N: rows of the feature table (the catalogue)")
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--json", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "agg_probe measures on the GPU only"
dev = torch.device("cuda")


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return {"ms_median": statistics.median(times), "ms_min": min(times), "peak_bytes": torch.cuda.max_memory_allocated() - before}


def host_timed(fn, reps=3):
    """a whole module call from python lists, host clock around a device synchronise (the padding is host work)"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def alternating(f1, f2):
    """both paths timed twice, interleaved; the better median of each"""
    r = [timed(f1), timed(f2), timed(f1), timed(f2)]
    return min(r[0], r[2], key=lambda d: d["ms_median"]), min(r[1], r[3], key=lambda d: d["ms_median"])


N, C = a.rows, a.channels
rs = np.random.RandomState(0)
x = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).to(dev)
torch.manual_seed(0)
at, mp = A.AttentionAggregator(C).to(dev).eval(), A.MaxPoolingAggregator(C, C).to(dev).eval()
rows = []
with torch.no_grad():
    for B, T in ((N, 10), (N, 50), (1024, 10), (1024, 50)):
        nvalid_h = rs.randint(0, T + 1, size=B).astype(np.int32)
        nvalid_h[::7] = T
        ids_h = rs.randint(0, N, size=(B, T)).astype(np.int32)
        lists = [ids_h[i, :nvalid_h[i]].tolist() for i in range(B)]
        t0 = time.perf_counter()
        ids, nvalid = A._pad_dev(lists, x)
        torch.cuda.synchronize()
        pad_ms = (time.perf_counter() - t0) * 1e3
        kept = int(nvalid_h.sum())
        gather_bytes = 4 * C * kept
        for name, m, args in (("attention", at, (x, ids, nvalid, x)), ("maxpool", mp, (x, ids, nvalid))):
            o_hip, o_torch = m._hip_padded(*args), m._torch_padded(*args)
            err = float((o_hip - o_torch).abs().max())
            assert err <= 1e-5 * float(o_torch.abs().max()) + 2e-6, (name, B, T, err)
            del o_hip, o_torch
            hip, plain = alternating(lambda: m._hip_padded(*args), lambda: m._torch_padded(*args))
            e2e_hip, e2e_torch = host_timed(lambda: m(x, lists)), host_timed(lambda: m._forward_torch(x, lists))
            if name == "attention":
                W1 = at.attention[0].weight
                u, v = dense.linear(x[:B], W1[:, :C], at.attention[0].bias), dense.linear(x, W1[:, C:])
                w2 = at.attention[2].weight.reshape(-1)
                kern = timed(lambda: sampling.attention_weights(u, v, w2, ids, nvalid))
                kname = "ps_attention_weights"
                del u, v
            else:
                t = dense.linear(x, mp.mlp[0].weight, mp.mlp[0].bias, relu=True)
                kern = timed(lambda: sampling.gather_max(t, ids, nvalid))
                kname = "ps_gather_max"
                del t
            row = {"aggregator": name, "B": B, "N": N, "C": C, "T": T, "kept_slots": kept, "pad_ms": pad_ms,
                   "hip_ms_median": hip["ms_median"], "hip_ms_min": hip["ms_min"], "hip_peak_bytes": hip["peak_bytes"],
                   "torch_ms_median": plain["ms_median"], "torch_ms_min": plain["ms_min"], "torch_peak_bytes": plain["peak_bytes"],
                   "torch_over_hip": plain["ms_median"] / hip["ms_median"],
                   "forward_ms_median": e2e_hip, "forward_torch_ms_median": e2e_torch, "max_abs_diff": err, "kernel": kname,
                   "kernel_ms_median": kern["ms_median"], "kernel_gather_bytes": gather_bytes,
                   "kernel_gather_GBps": gather_bytes / (kern["ms_median"] * 1e-3) / 1e9}
            rows.append(row)
            print(f"{name:9s} B={B:6d} T={T:2d}: hip {hip['ms_median']:8.3f} ms  torch {plain['ms_median']:8.3f} ms  x{row['torch_over_hip']:6.1f}"
                  f"  | from lists {e2e_hip:.1f} vs {e2e_torch:.1f} ms | {kname} {kern['ms_median']:.4f} ms, {row['kernel_gather_GBps']:.0f} GB/s | peak {hip['peak_bytes'] / 2**20:.0f} vs"
                  f" {plain['peak_bytes'] / 2**20:.0f} MiB", file=sys.stderr)
out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rows": rows}
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(out, open(a.json, "w"), indent=1)
print(json.dumps(out))
