"""The node2vec-biased walk against the first-order walk at the catalogue shape: RandomWalkSampler.sample_batches over all 59 047
items of bench.py's default synthetic catalogue (SYN-25M), W = 100, L = 2, T = 10, two layers, Philox, (p, q) = (0.25, 4) against
(1, 1) on one graph in one process.

    python tools/biased_walk_probe.py

Wall time of the call with a device synchronisation after one warm-up call: minimum and median of 20 unbiased and 3 biased calls;
then the kernel times of one biased call (native.KernelTimer), which give ps_paths_topk's share.  DESIGN.md, "Biased walks"."""
import os
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "movie-recommendation-engine_amd"))
import torch
from pinsage_hip import synth, native as nv
from pinsage_hip.graph import DeviceGraph
from utils.random_walk import RandomWalkSampler

dev = torch.device("cuda", 0)
src = synth.ML25M
U, M, R = src["num_users"], src["num_items"], src["num_ratings"]
ei, ew = synth.bipartite_ratings(U, M, R, seed=20240601, device=dev)
graph = DeviceGraph(ei, ew, device=dev)
del ei, ew
print("graph", graph.V, graph.E, "max degree", graph.max_degree, flush=True)


def timed(s, reps):
    s.sample_batches(range(M), 10, 2)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.sample_batches(range(M), 10, 2)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


plain = RandomWalkSampler.from_graph(graph, 2, 100, rng="philox", seed=42)
biased = RandomWalkSampler.from_graph(graph, 2, 100, rng="philox", seed=42, p=0.25, q=4.0)
tp = timed(plain, 20)
print("unbiased sample_batches ms (min / median):", tp[0], tp[len(tp) // 2], flush=True)
tb = timed(biased, 3)
print("biased   sample_batches ms (min / median):", tb[0], tb[len(tb) // 2], flush=True)
t = nv.KernelTimer()
nv.set_timer(t)
biased.sample_batches(range(M), 10, 2)
nv.set_timer(None)
for k, v in t.summary().items():
    print(k, v, flush=True)
