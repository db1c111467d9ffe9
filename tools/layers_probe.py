#!/usr/bin/env python3
"""GraphConvLayer: the HIP path (composed ps_linear + ps_bn_batch_stats + ps_bn_apply in training mode, one folded ps_linear in
eval mode) against the torch code of the same commit (`_forward_torch`), in ONE process on one GPU, alternating, under no_grad.
Per shape, mode and path: the median and minimum of `--reps` calls timed with HIP events after `--warmup` calls, and the rise of
torch's peak allocation over one call.  The two batch-norm kernels are also timed alone, `--inner` back-to-back launches between
one pair of events (a single launch of a few microseconds measures the event pair); their rate is over the algorithmic bytes --
ps_bn_batch_stats reads 4 M N, ps_bn_apply reads and writes 8 M N (in place, ReLU + L2 norm).  Prints one JSON line (and writes
it to --json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommendation-engine_amd"))
import torch                                                   # noqa: E402
from model import layers as L                                  # noqa: E402
from pinsage_hip import dense                                  # noqa: E402
from pinsage_hip import native as nv                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--json", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "layers_probe measures on the GPU only"
dev = torch.device("cuda")


def timed(fn, inner=1):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / inner)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return {"ms_median": statistics.median(times), "ms_min": min(times), "peak_bytes": torch.cuda.max_memory_allocated() - before}


def alternating(f1, f2):
    """both paths timed twice, interleaved; the better median of each"""
    r = [timed(f1), timed(f2), timed(f1), timed(f2)]
    return min(r[0], r[2], key=lambda d: d["ms_median"]), min(r[1], r[3], key=lambda d: d["ms_median"])


rows = []
with torch.no_grad():
    for M, cin, cout in ((59047, 256, 256), (1024, 256, 256)):
        torch.manual_seed(0)
        layer = L.GraphConvLayer(cin, cout).to(dev)
        x, nx = torch.randn(M, cin, device=dev), torch.randn(M, cin, device=dev)
        for training in (True, False):
            layer.train(training)
            assert layer._hip_serves(x, nx)
            o_hip, o_torch = layer._forward_hip(x, nx), layer._forward_torch(x, nx)
            err = float((o_hip - o_torch).abs().max())
            assert err <= 1e-5 * float(o_torch.abs().max()) + 2e-6, (M, training, err)
            del o_hip, o_torch
            hip, plain = alternating(lambda: layer._forward_hip(x, nx), lambda: layer._forward_torch(x, nx))
            row = {"M": M, "in": cin, "out": cout, "mode": "train" if training else "eval", "max_abs_diff": err,
                   "hip_ms_median": hip["ms_median"], "hip_ms_min": hip["ms_min"], "hip_peak_bytes": hip["peak_bytes"],
                   "torch_ms_median": plain["ms_median"], "torch_ms_min": plain["ms_min"], "torch_peak_bytes": plain["peak_bytes"],
                   "torch_over_hip": plain["ms_median"] / hip["ms_median"]}
            rows.append(row)
            print(f"M={M:6d} {row['mode']:5s}: hip {hip['ms_median']:8.4f} ms  torch {plain['ms_median']:8.4f} ms  x{row['torch_over_hip']:5.2f}"
                  f" | peak {hip['peak_bytes'] / 2**20:.1f} vs {plain['peak_bytes'] / 2**20:.1f} MiB | max |diff| {err:.1e}", file=sys.stderr)
        # the two kernels alone
        z = torch.randn(M, cout, device=dev)
        gamma, beta = layer.bn.weight.detach(), layer.bn.bias.detach()
        rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
        mean, _, scale = dense.batch_norm_stats(z, gamma, 1e-5, 0.1)
        var = torch.empty_like(mean)
        ws, wsb = nv.workspace("ps_bn_stats_workspace_bytes", dev, M, cout)
        st = nv.stream()                                       # the bare entry points over preallocated buffers: no allocator, no checks
        k_stats = timed(lambda: nv.call("ps_bn_batch_stats", nv.ptr(z), M, cout, nv.ptr(gamma), 1e-5, 0.1, nv.ptr(rm), nv.ptr(rv),
                                        nv.ptr(mean), nv.ptr(var), nv.ptr(scale), nv.ptr(ws), wsb, st), a.inner)
        k_apply = timed(lambda: nv.call("ps_bn_apply", nv.ptr(z), M, cout, nv.ptr(mean), nv.ptr(scale), nv.ptr(beta), 3, nv.ptr(z), st),
                        a.inner)
        for name, k, nbytes in (("ps_bn_batch_stats", k_stats, 4 * M * cout), ("ps_bn_apply", k_apply, 8 * M * cout)):
            row = {"kernel": name, "M": M, "N": cout, "ms_median": k["ms_median"], "ms_min": k["ms_min"], "bytes": nbytes,
                   "GBps": nbytes / (k["ms_median"] * 1e-3) / 1e9}
            rows.append(row)
            print(f"M={M:6d} {name:18s}: {k['ms_median'] * 1e3:8.2f} us per call ({a.inner} back to back), {row['GBps']:7.0f} GB/s", file=sys.stderr)
out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "rows": rows}
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(out, open(a.json, "w"), indent=1)
print(json.dumps(out))
