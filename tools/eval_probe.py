#!/usr/bin/env python3
"""utils.evaluation.evaluate_embeddings at run.py's shape (5 000 pairs x 59 047 items x D = 128) and at 10 000 x 59 047 x 256,
against two yardsticks, interleaved in one process:
  floor       bare ps_linear of the same shape (dense.linear(Q, E): writes the [nq, N] slab the rank epilogue never writes)
  torch       the torch-on-device composition: Q @ E^T, torch.sort descending, position of the ground truth
and the parts of the drop-in: ps_rank_count alone (the GEMM with the counting epilogue), dense.target_rank (gather + ps_row_dot +
ps_rank_count + the +1), evaluate_embeddings end to end (host pairs -> device, ranks -> host, four hit rates and the MRR).
One JSON line per shape: best-of-rounds milliseconds per leg, and how many ranks the torch composition gives differently
(torch's matmul sums in another order: only near-ties can differ)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommendation-engine_amd"))
import torch  # noqa: E402

from pinsage_hip import dense  # noqa: E402
from utils import evaluation as ev  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()
dev = torch.device("cuda")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_ranks(E, q, gt, chunk=2500):
    out = []
    for s in range(0, q.numel(), chunk):
        S = E.index_select(0, q[s:s + chunk]) @ E.t()
        idx = torch.sort(S, dim=1, descending=True).indices
        out.append((idx == gt[s:s + chunk, None]).int().argmax(1) + 1)
    return torch.cat(out)


for nq, N, D in ((5000, 59047, 128), (10000, 59047, 256)):
    g = torch.Generator(device="cpu").manual_seed(nq + D)
    E = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(dev).contiguous()
    pairs = torch.randint(0, N, (nq, 2), generator=g, dtype=torch.int64)
    test_data = {"positive_pairs": pairs}
    q, gt = pairs[:, 0].to(dev), pairs[:, 1].to(dev)
    Q = E.index_select(0, q).contiguous()
    thr = dense.row_dot(E, q, E, gt)
    count = torch.zeros(nq, dtype=torch.int64, device=dev)
    legs = {
        "floor_ps_linear": lambda: dense.linear(Q, E),
        "ps_rank_count": lambda: dense.rank_count(E, Q, thr, gt, count=count.zero_()),
        "target_rank": lambda: dense.target_rank(E, q, gt),
        "evaluate_embeddings": lambda: ev.evaluate_embeddings(E, test_data),
        "torch_matmul_sort": lambda: torch_ranks(E, q, gt),
    }
    best = {k: float("inf") for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            best[k] = min(best[k], timed(fn, a.reps if k != "torch_matmul_sort" else 2))
    ours = dense.target_rank(E, q, gt)
    theirs = torch_ranks(E, q, gt)
    flops = 2.0 * nq * N * D
    print(json.dumps({
        "shape": {"pairs": nq, "items": N, "D": D},
        "ms": {k: round(v, 4) for k, v in best.items()},
        "tflops": {k: round(flops / (best[k] * 1e-3) / 1e12, 1) for k in ("floor_ps_linear", "ps_rank_count")},
        "rank_count_vs_floor": round(best["ps_rank_count"] / best["floor_ps_linear"], 3),
        "torch_rank_mismatches": int((ours != theirs).sum()),
    }), flush=True)
