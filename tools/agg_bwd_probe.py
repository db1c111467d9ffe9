#!/usr/bin/env python3
"""Neighbour gathers under autograd: forward + backward time and peak memory of three modules with (a) the HIP backward
(sampling.grad_method = "hip": ps_pool_weights, ps_gather_bwd, ps_gather_max_arg, ps_attention_bwd_rows / _cols) and (b) the torch
code that served before (sampling.grad_method = "torch"), in ONE process on one GPU, interleaved.  Per line: the median of
`--reps` single forward + backward passes timed with HIP events after `--warmup` passes, the spread (min .. max) of the same
passes, and the rise of torch's peak allocation over one pass.  The comparison is (a) against (b), never against an earlier
state of the library.  Also: the share of the HIP backward spent in sampling.slot_lists (the transposition, torch ops)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommendation-engine_amd"))
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from model import aggregators as A                             # noqa: E402
from model.pinsage import PinSage                              # noqa: E402
from pinsage_hip import native as nv                           # noqa: E402
from pinsage_hip import sampling                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--small", action="store_true", help="a tenth of the catalogue shape (a quick look)")
a = ap.parse_args()
dev = torch.device("cuda")


def measure(step, leaves, params):
    def clear():
        for t in leaves:
            t.grad = None
        for p in params:
            p.grad = None
    for _ in range(a.warmup):
        clear()
        step().backward()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        clear()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        step().backward()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    clear()
    return dict(ms_median=statistics.median(times), ms_min=min(times), ms_max=max(times), peak_bytes=peak)


def slot_lists_share(ids, nvalid, n_rows, total_ms):
    """median time of sampling.slot_lists alone, as a share of a whole forward + backward pass"""
    times = []
    for i in range(a.warmup + a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        sampling.slot_lists(ids, nvalid, n_rows)
        e.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(s.elapsed_time(e))
    ms = statistics.median(times)
    return ms, ms / total_ms


def skewed_ids(rs, B, T, N):
    """ids with a popular head (id = floor(N r^3): row 0 is named by about N^(-1/3) of all slots), every slot kept"""
    return np.minimum((N * rs.random_sample((B, T)) ** 3).astype(np.int64), N - 1).astype(np.int32)


rows = []
rs = np.random.RandomState(7)
scale = 10 if a.small else 1

# ---- PinSage, pooled branch: B = N = 59 047, H = 256, T = 10, gradient to the parameters and to x ----
N, H, T = 59047 // scale, 256, 10
x = torch.randn(N, H, device=dev).requires_grad_(True)
torch.manual_seed(1)
model = PinSage(H, H, H, num_layers=2).to(dev)
batches = []
for _ in range(2):
    ids = torch.from_numpy(skewed_ids(rs, N, T, N)).to(dev)
    counts = torch.from_numpy(rs.randint(1, 30, size=(N, T)).astype(np.int32)).to(dev)
    batches.append(sampling.NeighborBatch(ids, counts, torch.full((N,), T, dtype=torch.int32, device=dev)))
nbs = [sampling.LazyNeighborList(b, "ids") for b in batches]
wts = [sampling.LazyNeighborList(b, "weights") for b in batches]
lines = [("PinSage pooled branch", (N, N, H, T), lambda: model(x, None, nbs, wts).square().sum(), [x], list(model.parameters()),
          (batches[0].ids, batches[0].nvalid, N))]

# ---- the two aggregators: B = N = 4096, C = 64, T = 32 ----
Na, C, Ta = 4096 // scale, 64, 32
xa = torch.randn(Na, C, device=dev).requires_grad_(True)
nb_list = rs.randint(0, Na, size=(Na, Ta)).tolist()
torch.manual_seed(2)
at, mp = A.AttentionAggregator(C).to(dev), A.MaxPoolingAggregator(C, C).to(dev)
ids_a, nvalid_a = A._pad_dev(nb_list, xa)
# the padded tensors are made once, outside the timed region: the list -> tensor conversion is the same host work either way
lines.append(("AttentionAggregator", (Na, Na, C, Ta),
              lambda: (at._hip_tape(xa, ids_a, nvalid_a, xa) if sampling.grad_method == "hip"
                       else at._torch_padded(xa, ids_a, nvalid_a, xa)).square().sum(), [xa], list(at.parameters()),
              (ids_a, nvalid_a, Na)))
lines.append(("MaxPoolingAggregator", (Na, Na, C, Ta),
              lambda: (mp._hip_tape(xa, ids_a, nvalid_a) if sampling.grad_method == "hip"
                       else mp._torch_padded(xa, ids_a, nvalid_a)).square().sum(), [xa], list(mp.parameters()),
              (ids_a, nvalid_a, Na)))

print(f"SEG = {nv.lib().ps_gather_bwd_segment()}; {a.reps} passes after {a.warmup} warm-ups; ms = median [min .. max]")
for name, shape, step, leaves, params, lists in lines:
    res = {}
    for method in ("hip", "torch"):
        sampling.grad_method = method
        res[method] = measure(step, leaves, params)
    sampling.grad_method = "hip"
    sl_ms, sl_share = slot_lists_share(*lists, res["hip"]["ms_median"])
    h, t = res["hip"], res["torch"]
    print(f"{name:22s} B,N,H,T={shape} | hip {h['ms_median']:8.3f} [{h['ms_min']:.3f} .. {h['ms_max']:.3f}] ms, "
          f"{h['peak_bytes'] / 2 ** 20:8.1f} MiB | torch {t['ms_median']:8.3f} [{t['ms_min']:.3f} .. {t['ms_max']:.3f}] ms, "
          f"{t['peak_bytes'] / 2 ** 20:8.1f} MiB | ratio {h['ms_median'] / t['ms_median']:.2f} | "
          f"slot_lists {sl_ms:.3f} ms = {100 * sl_share:.0f} % of a hip pass (one call; a pass makes one per pooled layer)")
    rows.append({"module": name, "B": shape[0], "N": shape[1], "H": shape[2], "T": shape[3], "hip": h, "torch": t,
                 "slot_lists_ms": sl_ms, "slot_lists_share_of_pass": sl_share, "segment": nv.lib().ps_gather_bwd_segment()})
if a.json:
    with open(a.json, "w") as f:
        json.dump(rows, f, indent=1)
